"""Encoder -- mirror of ``pfv_rs::enc::Encoder`` (src/enc.rs:12-188).

``Encoder(writer, width, height, framerate, quality, ctx)``: the reference's ``num_threads`` slot is the
:class:`Context` (device + stream).  ``writer`` is any object with ``write(bytes)``; like the reference the header
is written on construction, one packet per ``encode_*`` call, the EOF packet on ``finish()`` (also on close /
garbage collection if the caller did not finish, src/enc.rs:28-34).
"""
from __future__ import annotations

import ctypes

from . import _lib
from .context import Context, ptr
from .frame import VideoFrame


class Encoder:
    def __init__(self, writer, width: int, height: int, framerate: int, quality: int | None, ctx: Context, device_entropy: bool = True,
                 frame_report: bool = False, qualities=None, iframe_budget: int = 0, iframe_quality_floor: float = 0.0,
                 pframe_quality_floor: float = 0.0, frame_ssim: bool = False, iframe_ssim_floor: float = 0.0, pframe_ssim_floor: float = 0.0):
        """``qualities=[...]`` (next to ``quality=None``): a quality ladder -- 1..11 values in 0..10, strictly ascending (towards coarser
        quantisers); the header carries the tables of every rung and ``set_rung`` / ``set_rate`` choose per frame.  ``iframe_budget``: see
        ``set_iframe_budget``; ``iframe_quality_floor``: see ``set_iframe_quality_floor``; ``pframe_quality_floor``: see
        ``set_pframe_quality_floor``; ``iframe_ssim_floor`` / ``pframe_ssim_floor``: see ``set_iframe_ssim_floor`` / ``set_pframe_ssim_floor``"""
        self.ctx, self.writer = ctx, writer
        self.width, self.height = int(width), int(height)
        h = ctypes.c_void_p()
        if qualities is None:
            assert 0 <= quality <= 10                               # src/enc.rs:38
            ctx.check(ctx._lib.pfv_encoder_create(ctx.handle, self.width, self.height, int(framerate), int(quality), ctypes.byref(h)))
        else:
            assert quality is None, "give quality or qualities, not both"
            q = (ctypes.c_int * len(qualities))(*[int(x) for x in qualities])
            ctx.check(ctx._lib.pfv_encoder_create_ladder(ctx.handle, self.width, self.height, int(framerate), q, len(qualities), ctypes.byref(h)))
        self.handle = h
        # packet payloads from the device entropy stage (default) or the host serialisers: same bytes
        ctx.check(ctx._lib.pfv_encoder_set_device_entropy(h, 1 if device_entropy else 0))
        # frame_report: every encode_* call also measures its frame against the reconstruction it leaves behind (last_report); same bytes
        if frame_report:
            ctx.check(ctx._lib.pfv_encoder_set_frame_report(h, 1))
        # frame_ssim: a switch of its own -- the structural similarity of the same pair of frames (last_ssim); same bytes
        if frame_ssim:
            ctx.check(ctx._lib.pfv_encoder_set_frame_ssim(h, 1))
        if iframe_budget:
            ctx.check(ctx._lib.pfv_encoder_set_iframe_budget(h, int(iframe_budget)))
        if iframe_quality_floor:
            ctx.check(ctx._lib.pfv_encoder_set_iframe_quality_floor(h, float(iframe_quality_floor)))
        if pframe_quality_floor:
            ctx.check(ctx._lib.pfv_encoder_set_pframe_quality_floor(h, float(pframe_quality_floor)))
        if iframe_ssim_floor:
            ctx.check(ctx._lib.pfv_encoder_set_iframe_ssim_floor(h, float(iframe_ssim_floor)))
        if pframe_ssim_floor:
            ctx.check(ctx._lib.pfv_encoder_set_pframe_ssim_floor(h, float(pframe_ssim_floor)))
        self.finished = False
        ctx._sessions.add(self)
        self._flush()                                               # header (src/enc.rs:70)

    def _flush(self):
        # the library keeps only what has not been handed over yet (the reference writes each packet through, src/enc.rs:190-235)
        data, n = ctypes.c_void_p(), ctypes.c_size_t()
        self.ctx.check(self.ctx._lib.pfv_encoder_drain(self.handle, ctypes.byref(data), ctypes.byref(n)))
        if n.value:
            self.writer.write(ctypes.string_at(data.value, n.value))

    def set_input_rgb(self, on=True, fmt="rgb8", chroma="point"):
        """the encode_* / probe_* methods take one tight picture instead of a :class:`VideoFrame`: a uint8 array [height, width, 3 or 4] in
        fmt "rgb8" / "rgba8" / "bgra8"; chroma "point" (the reference's) or "box" (pfv_encoder_set_input_rgb)"""
        from .quality import chroma_mode, pix_format, rgb_shape
        m = pix_format(fmt)
        self.ctx.check(self.ctx._lib.pfv_encoder_set_input_rgb(self.handle, 1 if on else 0, m, chroma_mode(chroma)))
        self._rgb_format = m if on else None
        self._input_shapes()

    def set_input_size(self, src_width=0, src_height=0, kind="bicubic"):
        """the encode_* / probe_* methods take frames -- under set_input_rgb pictures -- of src_width x src_height, resized on the device to the
        encoder's size with kind "bilinear" / "bicubic" / "lanczos3"; src_width 0 switches it off (pfv_encoder_set_input_size)"""
        from .scale import scale_kind
        self.ctx.check(self.ctx._lib.pfv_encoder_set_input_size(self.handle, int(src_width or 0), int(src_height or 0), scale_kind(kind)))
        self._in_size = (int(src_width), int(src_height)) if src_width else None
        self._input_shapes()

    def set_denoise(self, on=True, spatial=(0, 0, 0), temporal=(0, 0, 0)):
        """the noise filter as the last input stage (behind set_input_rgb and set_input_size): strengths per plane (Y, U, V), 0 .. 16; the
        encode_* methods commit the filter's state, the probe_* methods do not (pfv_encoder_set_denoise)"""
        from .denoise import strengths
        s, t = strengths(spatial), strengths(temporal)
        self.ctx.check(self.ctx._lib.pfv_encoder_set_denoise(self.handle, 1 if on else 0, ptr(s), ptr(t)))

    def set_scene_cut(self, on=True, threshold_q8: int | None = None, radius: int | None = None, min_interval: int = 0):
        """scene-cut detection on the staged frame of every encode_* (committed) and probe_* (uncommitted) call; encode_frame then writes an
        i-frame where the score reaches threshold_q8 and min_interval frames have followed the last i-frame, and works in "full" / "hier"
        search mode too (pfv_encoder_set_scene_cut)"""
        from .scene import RADIUS_DEFAULT, THRESHOLD_DEFAULT
        self.ctx.check(self.ctx._lib.pfv_encoder_set_scene_cut(self.handle, 1 if on else 0, int(THRESHOLD_DEFAULT if threshold_q8 is None else threshold_q8),
                                                               int(RADIUS_DEFAULT if radius is None else radius), int(min_interval)))

    @property
    def last_scene(self):
        """SceneStats of the last call that measured a frame (pfv_encoder_last_scene); PfvError(PFV_ERR_STATE) when the switch is off or no
        frame has been measured"""
        import numpy as np
        from .scene import STATS_DTYPE, SceneStats
        r = np.zeros(1, dtype=STATS_DTYPE)
        self.ctx.check(self.ctx._lib.pfv_encoder_last_scene(self.handle, ptr(r)))
        return SceneStats.from_record(r[0])

    def set_motion_search(self, mode="fourstep", radius: int = 0):
        """the motion search of the p-frames that follow: "fourstep", "full" with a radius of 1..15 or "hier" with an even radius of 2..62
        (pfv_encoder_set_motion_search); full and hier mode exclude the p-frame probe, the p-frame floors and -- without set_scene_cut --
        encode_frame"""
        from ._lib import search_mode
        self.ctx.check(self.ctx._lib.pfv_encoder_set_motion_search(self.handle, search_mode(mode), int(radius)))

    def _input_shapes(self):
        from .quality import rgb_shape
        w, h = getattr(self, "_in_size", None) or (self.width, self.height)
        m = getattr(self, "_rgb_format", None)
        self._rgb_shape = rgb_shape(self.ctx, w, h, m) if m is not None else None

    def _input(self, frame):
        """the (y, u, v) of a C call: the frame's planes, or under set_input_rgb (picture, NULL, NULL)"""
        if getattr(self, "_rgb_shape", None):
            import numpy as np
            self._picture = np.ascontiguousarray(frame, dtype=np.uint8)        # alive until the call returns
            assert self._picture.shape == self._rgb_shape, (self._picture.shape, self._rgb_shape)
            return ptr(self._picture), None, None
        return ptr(frame.plane_y.pixels), ptr(frame.plane_u.pixels), ptr(frame.plane_v.pixels)

    def _check_frame(self, frame: VideoFrame):
        if getattr(self, "_rgb_shape", None):
            assert not self.finished
            return
        assert (frame.width, frame.height) == (getattr(self, "_in_size", None) or (self.width, self.height))  # src/enc.rs:76-79
        assert frame.plane_y.width == frame.width and frame.plane_y.height == frame.height
        assert frame.plane_u.width == frame.width // 2 and frame.plane_u.height == frame.height // 2
        assert frame.plane_v.width == frame.width // 2 and frame.plane_v.height == frame.height // 2
        assert not self.finished                                                                          # src/enc.rs:80

    def encode_iframe(self, frame: VideoFrame):
        self._check_frame(frame)
        self.ctx.check(self.ctx._lib.pfv_encoder_encode_iframe(self.handle, *self._input(frame)))
        self._flush()

    def encode_pframe(self, frame: VideoFrame):
        self._check_frame(frame)
        self.ctx.check(self.ctx._lib.pfv_encoder_encode_pframe(self.handle, *self._input(frame)))
        self._flush()

    def encode_dropframe(self):
        assert not self.finished
        self.ctx.check(self.ctx._lib.pfv_encoder_encode_dropframe(self.handle))
        self._flush()

    # quality ladder -------------------------------------------------------------------------------------------------
    @property
    def n_rungs(self) -> int:
        return int(self.ctx._lib.pfv_encoder_rungs(self.handle))

    def set_rung(self, rung: int):
        """the rung of the frames that follow"""
        self.ctx.check(self.ctx._lib.pfv_encoder_set_rung(self.handle, int(rung)))

    @property
    def rung(self) -> int:
        """the rung of the last frame written; before the first frame the current rung"""
        return int(self.ctx._lib.pfv_encoder_rung(self.handle))

    def set_rate(self, pframe_budget: int = 0):
        """byte budget per p-frame payload (0: off): a p-frame over it moves the next frame one rung coarser, one at half the budget or
        less one rung finer (pfv_encoder_set_rate)"""
        self.ctx.check(self.ctx._lib.pfv_encoder_set_rate(self.handle, int(pframe_budget)))

    def set_iframe_budget(self, iframe_budget: int = 0):
        """byte budget per i-frame payload (0: off): encode_iframe probes the frame and encodes it at the finest rung whose payload fits,
        the coarsest if none does; that rung becomes the current rung (pfv_encoder_set_iframe_budget)"""
        self.ctx.check(self.ctx._lib.pfv_encoder_set_iframe_budget(self.handle, int(iframe_budget)))

    def probe_iframe(self, frame: VideoFrame):
        """payload bytes of `frame` as an i-frame at every rung, uint32 [n_rungs] (0xffffffff: not encodable at that rung); the stream, the
        encoder's reference and the rung stay as they are"""
        import numpy as np
        self._check_frame(frame)
        sizes = np.zeros(self.n_rungs, dtype=np.uint32)
        self.ctx.check(self.ctx._lib.pfv_encoder_probe_iframe(self.handle, *self._input(frame), ptr(sizes)))
        return sizes

    def set_iframe_quality_floor(self, min_psnr_yuv: float = 0.0):
        """PSNR-YUV floor in dB per i-frame (0: off; inf: the best-looking rung that fits): encode_iframe probes size and squared error at
        every rung and takes, of the rungs within the i-frame budget that reach the floor, the one with the fewest bytes -- if none does,
        the one with the smallest error; that rung becomes the current rung (pfv_encoder_set_iframe_quality_floor)"""
        self.ctx.check(self.ctx._lib.pfv_encoder_set_iframe_quality_floor(self.handle, float(min_psnr_yuv)))

    def probe_iframe_rd(self, frame: VideoFrame):
        """(sizes uint32 [n_rungs], sse uint64 [n_rungs, 3]) of `frame` as an i-frame at every rung: payload bytes as probe_iframe and the
        squared error per plane a frame report would show at that rung; the stream, the encoder's reference and the rung stay as they are"""
        import numpy as np
        self._check_frame(frame)
        sizes, sse = np.zeros(self.n_rungs, dtype=np.uint32), np.zeros((self.n_rungs, 3), dtype=np.uint64)
        self.ctx.check(self.ctx._lib.pfv_encoder_probe_iframe_rd(self.handle, *self._input(frame), ptr(sizes), ptr(sse)))
        return sizes, sse

    def probe_pframe(self, frame: VideoFrame):
        """payload bytes of `frame` as a p-frame against the encoder's reference at every rung, uint32 [n_rungs] (0xffffffff: not encodable at
        that rung); the stream, the reference and the rung stay as they are.  PfvError(PFV_ERR_STATE) when poisoned or finished"""
        import numpy as np
        sizes = np.zeros(self.n_rungs, dtype=np.uint32)
        self.ctx.check(self.ctx._lib.pfv_encoder_probe_pframe(self.handle, *self._input(frame), ptr(sizes)))
        return sizes

    def probe_pframe_rd(self, frame: VideoFrame):
        """(sizes uint32 [n_rungs], sse uint64 [n_rungs, 3]) of `frame` as a p-frame against the encoder's reference at every rung: payload
        bytes as probe_pframe and the squared error per plane a frame report would show at that rung; the stream, the reference and the rung
        stay as they are.  PfvError(PFV_ERR_STATE) when poisoned or finished"""
        import numpy as np
        sizes, sse = np.zeros(self.n_rungs, dtype=np.uint32), np.zeros((self.n_rungs, 3), dtype=np.uint64)
        self.ctx.check(self.ctx._lib.pfv_encoder_probe_pframe_rd(self.handle, *self._input(frame), ptr(sizes), ptr(sse)))
        return sizes, sse

    def set_pframe_quality_floor(self, min_psnr_yuv: float = 0.0):
        """PSNR-YUV floor in dB per p-frame (0: off; inf: the best-looking rung that fits): encode_pframe probes size and squared error at
        every rung and takes, of the rungs within the set_rate budget (a hard cap here) that reach the floor, the one with the fewest bytes
        -- if none does, the one with the smallest error; encode_frame then weighs that p-frame against the i-frame by the same measure
        (pfv_encoder_set_pframe_quality_floor)"""
        self.ctx.check(self.ctx._lib.pfv_encoder_set_pframe_quality_floor(self.handle, float(min_psnr_yuv)))

    # SSIM probe and floors ------------------------------------------------------------------------------------------
    def _probe_ssim(self, fn, frame: VideoFrame):
        import numpy as np
        sizes, sse = np.zeros(self.n_rungs, dtype=np.uint32), np.zeros((self.n_rungs, 3), dtype=np.uint64)
        q24 = np.zeros((self.n_rungs, 3), dtype=np.int64)
        self.ctx.check(fn(self.handle, *self._input(frame), ptr(sizes), ptr(sse), ptr(q24)))
        return sizes, sse, q24

    def probe_iframe_ssim(self, frame: VideoFrame):
        """(sizes uint32 [n_rungs], sse uint64 [n_rungs, 3], ssim_q24 int64 [n_rungs, 3]) of `frame` as an i-frame at every rung:
        probe_iframe_rd's results and the SSIM sums per plane that last_ssim would show at that rung; nothing changes"""
        self._check_frame(frame)
        return self._probe_ssim(self.ctx._lib.pfv_encoder_probe_iframe_ssim, frame)

    def probe_pframe_ssim(self, frame: VideoFrame):
        """the same as a p-frame against the encoder's reference: probe_pframe_rd's results and the SSIM sums; nothing changes.
        PfvError(PFV_ERR_STATE) when poisoned or finished"""
        return self._probe_ssim(self.ctx._lib.pfv_encoder_probe_pframe_ssim, frame)

    def set_iframe_ssim_floor(self, min_ssim: float = 0.0):
        """floor on the frame's mean SSIM per i-frame (0: off; 1: the best-looking rung that fits): encode_iframe runs the SSIM probe and
        takes, of the rungs within the i-frame budget that reach this floor and the PSNR floor, the one with the fewest bytes -- if none
        does, the one with the largest SSIM; that rung becomes the current rung (pfv_encoder_set_iframe_ssim_floor)"""
        self.ctx.check(self.ctx._lib.pfv_encoder_set_iframe_ssim_floor(self.handle, float(min_ssim)))

    def set_pframe_ssim_floor(self, min_ssim: float = 0.0):
        """the same per p-frame, within the set_rate budget (a hard cap here); encode_frame then weighs that p-frame against the i-frame
        by the same measure (pfv_encoder_set_pframe_ssim_floor)"""
        self.ctx.check(self.ctx._lib.pfv_encoder_set_pframe_ssim_floor(self.handle, float(min_ssim)))

    def set_pframe_probe(self, on: bool = True):
        """on, with a set_rate budget and more than one rung: encode_pframe probes the frame and encodes it at the finest rung whose payload
        fits the budget, the coarsest if none does -- a hard budget instead of set_rate's soft rule (pfv_encoder_set_pframe_probe)"""
        self.ctx.check(self.ctx._lib.pfv_encoder_set_pframe_probe(self.handle, 1 if on else 0))

    def set_gop(self, max_interval: int = 0):
        """encode_frame forces an i-frame once `max_interval` frames (drop frames included) have followed the last one; 0: never"""
        self.ctx.check(self.ctx._lib.pfv_encoder_set_gop(self.handle, int(max_interval)))

    def encode_frame(self, frame: VideoFrame) -> int:
        """the frame's type chosen by the probes (pfv_encoder_encode_frame, include/pfv_hip_ext.h) -> 1 i-frame, 2 p-frame, 3 drop frame"""
        self._check_frame(frame)
        t = ctypes.c_int(0)
        self.ctx.check(self.ctx._lib.pfv_encoder_encode_frame(self.handle, *self._input(frame), ctypes.byref(t)))
        self._flush()
        return int(t.value)

    @property
    def last_report(self):
        """FrameReport of the last encode_* call (pfv_encoder_frame_report); PfvError(PFV_ERR_STATE) when reports are off, nothing has
        been encoded yet or that call failed"""
        from .quality import FrameReport, FrameReportStruct
        r = FrameReportStruct()
        self.ctx.check(self.ctx._lib.pfv_encoder_frame_report(self.handle, ctypes.byref(r)))
        return FrameReport(int(r.type), int(r.packet_bytes), tuple(int(v) for v in r.sse), tuple(float(v) for v in r.psnr), float(r.psnr_yuv))

    @property
    def last_ssim(self):
        """FrameSsim of the last encode_* call (pfv_encoder_frame_ssim); PfvError(PFV_ERR_STATE) when frame_ssim is off, nothing has been
        encoded yet or that call failed"""
        from .quality import FrameSsim, FrameSsimStruct
        r = FrameSsimStruct()
        self.ctx.check(self.ctx._lib.pfv_encoder_frame_ssim(self.handle, ctypes.byref(r)))
        return FrameSsim(tuple(int(v) for v in r.q24), tuple(int(v) for v in r.windows), tuple(float(v) for v in r.ssim), float(r.ssim_all))

    def finish(self):
        assert not self.finished                                    # src/enc.rs:183
        self.ctx.check(self.ctx._lib.pfv_encoder_finish(self.handle))
        self.finished = True
        self._flush()

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            if not self.finished:                                   # impl Drop (src/enc.rs:28-34)
                self.finish()
            self.ctx._lib.pfv_encoder_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchEncoder:
    """``n`` independent streams of one geometry encoded together: one upload, one kernel launch per stage and one
    download per frame step for all of them (the reference runs one ``Encoder`` per stream, src/enc.rs:12-26).  Each
    writer receives exactly the bytes an ``Encoder`` of its own would have written.  The orchestration (copy stream for
    the next step's upload, payload collection, packet assembly) is the C++ ``pfv_batch_encoder``; this class marshals.

    The caller fills ``frames`` -- a page-locked ``[n, frame_bytes]`` uint8 array, one packed Y|U|V frame per stream; two
    such arrays alternate, fetch the attribute again after every step -- and calls ``encode_iframes()`` /
    ``encode_pframes()``; or passes its own ``[n, frame_bytes]`` array to them.  Packets reach the writers one step late;
    ``finish()`` flushes and writes the EOF packets."""

    def __init__(self, writers, width: int, height: int, framerate: int, quality: int, ctx: Context):
        import numpy as np
        assert 0 <= quality <= 10 and len(writers) >= 1
        self.ctx, self.writers, self.n = ctx, list(writers), len(writers)
        self.width, self.height = int(width), int(height)
        self.frame_bytes = int(ctx._lib.pfv_frame_bytes(width, height))
        self.finished = False
        self._np = np

        self._write_error = None          # ctypes swallows exceptions raised inside a callback: keep the first one, stop
        #                                   writing (nothing after a failed write may reach any writer out of order) and re-raise it
        #                                   when the C call returns -- the reference propagates every write error (`?`, src/enc.rs:190-235)

        def on_write(_user, stream, data, length):
            if self._write_error is not None:
                return
            try:
                self.writers[stream].write(ctypes.string_at(data, length))
            except BaseException as e:      # noqa: BLE001 -- re-raised by _raise_write_error
                self._write_error = e
        self._cb = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t)(on_write)
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.pfv_batch_encoder_create(ctx.handle, self.width, self.height, int(framerate), int(quality), self.n,
                                                    ctypes.cast(self._cb, ctypes.c_void_p), None, ctypes.byref(h)))
        self.handle = h
        ctx._sessions.add(self)

    @property
    def frames(self):
        """the page-locked [n, frame_bytes] array to fill for the next step"""
        p = self.ctx._lib.pfv_batch_encoder_frames(self.handle)
        return self._np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(self.n, self.frame_bytes))

    def _step(self, pframe: bool, frames=None):
        assert not self.finished
        src = None
        if frames is not None:
            src = self._np.ascontiguousarray(frames, dtype=self._np.uint8)
            assert src.size == self.n * self.frame_bytes
        rc = self.ctx._lib.pfv_batch_encoder_encode(self.handle, 1 if pframe else 0, ptr(src) if src is not None else None)
        self._raise_write_error()
        self.ctx.check(rc)

    def _raise_write_error(self):
        """a writer failed inside the callback: the stream it belongs to is truncated, nothing more is written to any writer"""
        if self._write_error is not None:
            self.finished = True            # close() must not try to write EOF packets behind the hole
            raise self._write_error

    def encode_iframes(self, frames=None):
        self._step(False, frames)

    def encode_pframes(self, frames=None):
        self._step(True, frames)

    def flush(self):
        rc = self.ctx._lib.pfv_batch_encoder_flush(self.handle)
        self._raise_write_error()
        self.ctx.check(rc)

    def finish(self):
        assert not self.finished
        rc = self.ctx._lib.pfv_batch_encoder_finish(self.handle)
        self._raise_write_error()
        self.ctx.check(rc)
        self.finished = True

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            if not self.finished:
                self.finish()
            self.ctx._lib.pfv_batch_encoder_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _IoVec(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_size_t)]


class GopEncoder(Encoder):
    """:class:`Encoder` for one stream with the independent GOPs of the stream as the slots of every kernel launch
    (``pfv_gop_encoder``, include/pfv_hip.h): same calls, same ``.pfv`` bytes; a packet reaches the writer when its batch of
    ``max_gops`` groups is complete (or on ``flush()`` / ``finish()``).  ``encode_*frame`` also accept the three planes as flat
    uint8 arrays ``(y, u, v)`` -- e.g. views into page-locked memory (``Context.host_array``), which upload at PCIe rate."""

    def __init__(self, writer, width: int, height: int, framerate: int, quality: int, ctx: Context, max_gops: int = 8, max_gop_frames: int = 15,
                 payload_budget: int = 0, zero_copy: bool = False):
        """zero_copy: the writer receives memoryviews into the library's page-locked buffers (valid during the write() call only, which
        is all a file or a socket needs) instead of bytes copies"""
        assert 0 <= quality <= 10                                   # src/enc.rs:38
        self.ctx, self.writer, self.zero_copy = ctx, writer, zero_copy
        self.width, self.height = int(width), int(height)
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.pfv_gop_encoder_create(ctx.handle, self.width, self.height, int(framerate), int(quality), int(max_gops), int(max_gop_frames),
                                                  int(payload_budget), ctypes.byref(h)))
        self.handle = h
        self.finished = False
        ctx._sessions.add(self)
        self._flush()                                               # header (src/enc.rs:70)

    def _flush(self):
        # packet headers and payloads where they lie (pfv_gop_encoder_drain_iov): one write per segment, like the reference's W: Write
        iov, n = ctypes.c_void_p(), ctypes.c_size_t()
        self.ctx.check(self.ctx._lib.pfv_gop_encoder_drain_iov(self.handle, ctypes.byref(iov), ctypes.byref(n)))
        if not n.value:
            return
        segs = ctypes.cast(iov, ctypes.POINTER(_IoVec))
        for i in range(n.value):
            p, ln = segs[i].data, segs[i].len
            if self.zero_copy:      # a view into the library's page-locked memory, valid during this write() only
                self.writer.write(memoryview((ctypes.c_ubyte * ln).from_address(p)))
            else:
                self.writer.write(ctypes.string_at(p, ln))

    def _planes(self, frame):
        if isinstance(frame, VideoFrame):
            self._check_frame(frame)
            return ptr(frame.plane_y.pixels), ptr(frame.plane_u.pixels), ptr(frame.plane_v.pixels)
        y, u, v = frame
        assert not self.finished and y.size == self.width * self.height and u.size == v.size == (self.width // 2) * (self.height // 2)
        return ptr(y), ptr(u), ptr(v)

    def set_input_rgb(self, on=True, fmt="rgb8", chroma="point"):
        raise NotImplementedError("pfv_gop_encoder has no RGB switch: convert with pfv_frames_from_rgb_dev and use its _dev forms")

    def set_input_size(self, src_width=0, src_height=0, kind="bicubic"):
        raise NotImplementedError("pfv_gop_encoder has no resize switch: resize with pfv_scaler_run_dev and use its _dev forms")

    def encode_iframe(self, frame):
        self.ctx.check(self.ctx._lib.pfv_gop_encoder_encode_iframe(self.handle, *self._planes(frame)))
        self._flush()

    def encode_pframe(self, frame):
        self.ctx.check(self.ctx._lib.pfv_gop_encoder_encode_pframe(self.handle, *self._planes(frame)))
        self._flush()

    def set_motion_search(self, mode="fourstep", radius: int = 0):
        """the motion search of the batches submitted from now on: "fourstep", "full" with a radius of 1..15 or "hier" with an even radius
        of 2..62; refused while a batch is in flight (pfv_gop_encoder_set_motion_search)"""
        from ._lib import search_mode
        self.ctx.check(self.ctx._lib.pfv_gop_encoder_set_motion_search(self.handle, search_mode(mode), int(radius)))

    def set_frames_by_reference(self, on: bool = True):
        """device frames (encode_*_dev) are read where they lie instead of being copied into the batch: the caller keeps each frame valid and
        unchanged until its packet has reached the writer (or flush() / finish() returned).  pfv_gop_encoder_set_frames_by_reference."""
        self.ctx.check(self.ctx._lib.pfv_gop_encoder_set_frames_by_reference(self.handle, 1 if on else 0))

    def encode_iframe_dev(self, frame_dev: int):
        """a packed frame (Y | U | V) in DEVICE memory: pfv_gop_encoder_encode_iframe_dev.  STREAM-ORDERED on the context this encoder was created
        on, like every *_dev call: the frame is copied into the batch asynchronously on that context's stream and the call returns WITHOUT a host
        wait.  Whatever produces the frame, and whatever overwrites it afterwards, must be enqueued on the same context's stream (or ordered
        against it: Context.wait_event) -- a hipMemcpy from the host or a kernel on another stream right after the call races with the copy.
        The encoder must be closed before its context is."""
        assert not self.finished
        self.ctx.check(self.ctx._lib.pfv_gop_encoder_encode_iframe_dev(self.handle, ctypes.c_void_p(int(frame_dev))))
        self._flush()

    def encode_pframe_dev(self, frame_dev: int):
        """see encode_iframe_dev: stream-ordered on the encoder's context, no host wait"""
        assert not self.finished
        self.ctx.check(self.ctx._lib.pfv_gop_encoder_encode_pframe_dev(self.handle, ctypes.c_void_p(int(frame_dev))))
        self._flush()

    def encode_dropframe(self):
        assert not self.finished
        self.ctx.check(self.ctx._lib.pfv_gop_encoder_encode_dropframe(self.handle))

    def flush(self):
        """every frame handed over so far becomes packets at the writer now"""
        self.ctx.check(self.ctx._lib.pfv_gop_encoder_flush(self.handle))
        self._flush()

    def finish(self):
        assert not self.finished                                    # src/enc.rs:183
        self.ctx.check(self.ctx._lib.pfv_gop_encoder_finish(self.handle))
        self.finished = True
        self._flush()

    @property
    def batches(self) -> int:
        return int(self.ctx._lib.pfv_gop_encoder_batches(self.handle))

    def stats(self) -> dict:
        """host seconds so far, by what the object was waiting for (pfv_gop_encoder_stats)"""
        a = (ctypes.c_double * 7)()
        n = self.ctx._lib.pfv_gop_encoder_stats(self.handle, a, 7)
        return dict(zip(("upload_wait_s", "enqueue_s", "kernel_wait_s", "payload_download_s", "packet_assembly_s", "frames_by_reference", "batches_redone"),
                        list(a)[:n]))

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            if not self.finished:                                   # impl Drop (src/enc.rs:28-34)
                try:
                    self.finish()
                except _lib.PfvError:
                    pass                                            # a failed stream stays incomplete
            self.ctx._lib.pfv_gop_encoder_destroy(self.handle)
        self.handle = None
