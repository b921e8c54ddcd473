"""Device-resident encoder / decoder sessions: the hot-path half of ``enc::Encoder`` and
``dec::Decoder`` (src/enc.rs:12-173, src/dec.rs:15-224) for ``n_streams`` independent
streams per launch.  prev_frame / framebuffer stay in HBM between frames.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .context import Context, ptr


def qtables_from_quality(quality: int):
    """Encoder::new's table derivation (src/enc.rs:40-51) -> (intra_l, intra_c, inter_l, inter_c, px_err)."""
    lib = _lib.load()
    t = [np.zeros(64, dtype=np.int32) for _ in range(4)]
    pe = ctypes.c_float()
    rc = lib.pfv_qtables_from_quality(int(quality), ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), ctypes.byref(pe))
    _lib.check(None, rc)
    return t[0], t[1], t[2], t[3], float(pe.value)


class _Geometry:
    def __init__(self, width: int, height: int, n_streams: int):
        lib = _lib.load()
        self.width, self.height, self.n_streams = int(width), int(height), int(n_streams)
        self.frame_bytes = int(lib.pfv_frame_bytes(width, height))
        self.padded_frame_bytes = int(lib.pfv_padded_frame_bytes(width, height))
        self.total_blocks = int(lib.pfv_total_blocks(width, height))


class EncoderSession(_Geometry):
    def __init__(self, ctx: Context, width: int, height: int, quality: int | None, n_streams: int = 1, qualities=None):
        """``qualities=[...]`` (with ``quality=None``): a quality ladder, 1..11 values in 0..10, strictly ascending; ``set_rung`` picks the
        rung of the launches that follow"""
        super().__init__(width, height, n_streams)
        self.ctx = ctx
        h = ctypes.c_void_p()
        if qualities is None:
            ctx.check(ctx._lib.pfv_enc_session_create(ctx.handle, int(width), int(height), int(quality), int(n_streams),
                                                      ctypes.byref(h)))
        else:
            assert quality is None, "give quality or qualities, not both"
            q = (ctypes.c_int * len(qualities))(*[int(x) for x in qualities])
            ctx.check(ctx._lib.pfv_enc_session_create_ladder(ctx.handle, int(width), int(height), q, len(qualities), int(n_streams),
                                                             ctypes.byref(h)))
        self.handle = h
        ctx._sessions.add(self)

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            self.ctx._lib.pfv_enc_session_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # quality ladder ----------------------------------------------------
    @property
    def n_rungs(self) -> int:
        return int(self.ctx._lib.pfv_enc_session_rungs(self.handle))

    @property
    def rung(self) -> int:
        return int(self.ctx._lib.pfv_enc_session_rung(self.handle))

    def set_rung(self, rung: int):
        """the rung of the encode / pack launches that follow (all slots of a launch share it)"""
        self.ctx.check(self.ctx._lib.pfv_enc_session_set_rung(self.handle, int(rung)))

    # motion search ------------------------------------------------------
    def set_motion_search(self, mode="fourstep", radius: int = 0):
        """how the p-frame launches that follow choose their vectors: "fourstep" (the reference's search, the default), "full" with a
        radius of 1..15, every vector of the square, or "hier" with an even radius of 2..62, a coarse search at half size and a fine one
        round it (pfv_enc_session_set_motion_search); the p-frame probes are refused in full and hier mode"""
        from ._lib import search_mode
        self.ctx.check(self.ctx._lib.pfv_enc_session_set_motion_search(self.handle, search_mode(mode), int(radius)))

    @property
    def motion_search(self):
        """(mode, radius): PFV_SEARCH_FOURSTEP / PFV_SEARCH_FULL / PFV_SEARCH_HIER, and the radius (0 for four-step)"""
        m, r = ctypes.c_int(), ctypes.c_int()
        self.ctx.check(self.ctx._lib.pfv_enc_session_get_motion_search(self.handle, ctypes.byref(m), ctypes.byref(r)))
        return int(m.value), int(r.value)

    def coarse_vectors(self) -> np.ndarray:
        """the coarse level's vectors of the last p-frame launch, which was a "hier" one, over the current window: int8
        [slots, macroblocks, 2] in half-resolution pixels (pfv_enc_session_coarse_vectors; waits for the stream)"""
        out = np.zeros((getattr(self, "_win_count", self.n_streams), self.total_blocks, 2), np.int8)
        self.ctx.check(self.ctx._lib.pfv_enc_session_coarse_vectors(self.handle, out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
        return out

    HIER_STAGES = ("halve_src", "halve_ref", "coarse", "refine", "transform")

    def encode_pframe_hier_timed_dev(self, frames_dev: int, mv_dev: int, has_dev: int, coef_dev: int) -> dict:
        """encode_pframe_dev in "hier" mode with an event round every kernel: milliseconds per stage (pfv_enc_pframe_hier_timed_dev; waits)"""
        ms = (ctypes.c_float * 5)()
        self.ctx.check(self.ctx._lib.pfv_enc_pframe_hier_timed_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(mv_dev), ctypes.c_void_p(has_dev),
                                                                   ctypes.c_void_p(coef_dev), ms))
        return dict(zip(self.HIER_STAGES, (float(x) for x in ms)))

    # i-frame size probe -------------------------------------------------
    def probe_iframe(self, frames) -> np.ndarray:
        """payload bytes of every stream's frame as an i-frame at every rung, uint32 [n_streams, n_rungs], from one read of the frames
        (pfv_enc_probe_iframe); 0xffffffff: not encodable at that rung.  Leaves prev_frame and the rung alone."""
        f = self._frames(frames)
        sizes = np.zeros((self.n_streams, self.n_rungs), dtype=np.uint32)
        self.ctx.check(self.ctx._lib.pfv_enc_probe_iframe(self.handle, ptr(f), ptr(sizes)))
        return sizes

    def probe_iframe_dev(self, frames_dev: int, sizes_dev: int, stats_dev: int = 0):
        """asynchronous on the context's stream; sizes_dev uint32 [n_streams][n_rungs], stats_dev uint32 [n_streams][n_rungs][17] or 0.
        Honours the window and the frame stride."""
        self.ctx.check(self.ctx._lib.pfv_enc_probe_iframe_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(sizes_dev),
                                                              ctypes.c_void_p(stats_dev or 0)))

    # i-frame rate-distortion probe ---------------------------------------
    def probe_iframe_rd(self, frames):
        """(sizes uint32 [n_streams, n_rungs], sse uint64 [n_streams, n_rungs, 3]) of every stream's frame as an i-frame at every rung, from
        one read of the frames (pfv_enc_probe_iframe_rd): payload bytes as probe_iframe, squared error per plane (Y, U, V) against the
        reconstruction that rung would leave in prev_frame.  Leaves prev_frame and the rung alone."""
        f = self._frames(frames)
        sizes = np.zeros((self.n_streams, self.n_rungs), dtype=np.uint32)
        sse = np.zeros((self.n_streams, self.n_rungs, 3), dtype=np.uint64)
        self.ctx.check(self.ctx._lib.pfv_enc_probe_iframe_rd(self.handle, ptr(f), ptr(sizes), ptr(sse)))
        return sizes, sse

    def probe_iframe_rd_dev(self, frames_dev: int, sizes_dev: int, sse_dev: int, stats_dev: int = 0):
        """asynchronous on the context's stream; sizes_dev uint32 [n_streams][n_rungs], sse_dev uint64 [n_streams][n_rungs][3], stats_dev
        uint32 [n_streams][n_rungs][17] or 0.  Honours the window and the frame stride."""
        self.ctx.check(self.ctx._lib.pfv_enc_probe_iframe_rd_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(sizes_dev),
                                                                 ctypes.c_void_p(sse_dev), ctypes.c_void_p(stats_dev or 0)))

    # p-frame size probe -------------------------------------------------
    def probe_pframe(self, frames) -> np.ndarray:
        """payload bytes of every stream's frame as a p-frame against the current prev_frame at every rung, uint32 [n_streams, n_rungs], from
        one search and one transform (pfv_enc_probe_pframe); 0xffffffff: not encodable at that rung.  Leaves prev_frame and the rung alone."""
        f = self._frames(frames)
        sizes = np.zeros((self.n_streams, self.n_rungs), dtype=np.uint32)
        self.ctx.check(self.ctx._lib.pfv_enc_probe_pframe(self.handle, ptr(f), ptr(sizes)))
        return sizes

    def probe_pframe_dev(self, frames_dev: int, sizes_dev: int, stats_dev: int = 0):
        """asynchronous on the context's stream; sizes_dev uint32 [n_streams][n_rungs], stats_dev uint32 [n_streams][n_rungs][20] or 0 (16
        symbol counts, sum of coefficient sizes, coded macroblocks, macroblocks with a non-zero vector, header bits).  Honours the window and
        the frame stride."""
        self.ctx.check(self.ctx._lib.pfv_enc_probe_pframe_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(sizes_dev),
                                                              ctypes.c_void_p(stats_dev or 0)))

    # p-frame rate-distortion probe ---------------------------------------
    def probe_pframe_rd(self, frames):
        """(sizes uint32 [n_streams, n_rungs], sse uint64 [n_streams, n_rungs, 3]) of every stream's frame as a p-frame against the current
        prev_frame at every rung, from one search and one transform (pfv_enc_probe_pframe_rd): payload bytes as probe_pframe, squared error
        per plane (Y, U, V) against the reconstruction that rung would leave in prev_frame.  Leaves prev_frame and the rung alone."""
        f = self._frames(frames)
        sizes = np.zeros((self.n_streams, self.n_rungs), dtype=np.uint32)
        sse = np.zeros((self.n_streams, self.n_rungs, 3), dtype=np.uint64)
        self.ctx.check(self.ctx._lib.pfv_enc_probe_pframe_rd(self.handle, ptr(f), ptr(sizes), ptr(sse)))
        return sizes, sse

    def probe_pframe_rd_dev(self, frames_dev: int, sizes_dev: int, sse_dev: int, stats_dev: int = 0):
        """asynchronous on the context's stream; sizes_dev uint32 [n_streams][n_rungs], sse_dev uint64 [n_streams][n_rungs][3], stats_dev
        uint32 [n_streams][n_rungs][20] or 0.  Honours the window and the frame stride."""
        self.ctx.check(self.ctx._lib.pfv_enc_probe_pframe_rd_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(sizes_dev),
                                                                 ctypes.c_void_p(sse_dev), ctypes.c_void_p(stats_dev or 0)))

    # SSIM probe -----------------------------------------------------------
    def _probe_ssim(self, fn, frames):
        f = self._frames(frames)
        sizes = np.zeros((self.n_streams, self.n_rungs), dtype=np.uint32)
        sse = np.zeros((self.n_streams, self.n_rungs, 3), dtype=np.uint64)
        q24 = np.zeros((self.n_streams, self.n_rungs, 3), dtype=np.int64)
        self.ctx.check(fn(self.handle, ptr(f), ptr(sizes), ptr(sse), ptr(q24)))
        return sizes, sse, q24

    def probe_iframe_ssim(self, frames):
        """(sizes uint32 [n_streams, n_rungs], sse uint64 [n_streams, n_rungs, 3], ssim_q24 int64 [n_streams, n_rungs, 3]) of every stream's
        frame as an i-frame at every rung (pfv_enc_probe_iframe_ssim): probe_iframe_rd's results and the SSIM sums per plane (Y, U, V)
        against the reconstruction that rung would leave in prev_frame.  Leaves prev_frame and the rung alone."""
        return self._probe_ssim(self.ctx._lib.pfv_enc_probe_iframe_ssim, frames)

    def probe_iframe_ssim_dev(self, frames_dev: int, sizes_dev: int, sse_dev: int, ssim_q24_dev: int, stats_dev: int = 0):
        """asynchronous on the context's stream; as probe_iframe_rd_dev with ssim_q24_dev int64 [n_streams][n_rungs][3].  Honours the window
        and the frame stride."""
        self.ctx.check(self.ctx._lib.pfv_enc_probe_iframe_ssim_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(sizes_dev),
                                                                   ctypes.c_void_p(sse_dev), ctypes.c_void_p(ssim_q24_dev), ctypes.c_void_p(stats_dev or 0)))

    def probe_pframe_ssim(self, frames):
        """the same as p-frames against the current prev_frame (pfv_enc_probe_pframe_ssim): probe_pframe_rd's results and the SSIM sums"""
        return self._probe_ssim(self.ctx._lib.pfv_enc_probe_pframe_ssim, frames)

    def probe_pframe_ssim_dev(self, frames_dev: int, sizes_dev: int, sse_dev: int, ssim_q24_dev: int, stats_dev: int = 0):
        """asynchronous on the context's stream; as probe_pframe_rd_dev with ssim_q24_dev int64 [n_streams][n_rungs][3].  Honours the window
        and the frame stride."""
        self.ctx.check(self.ctx._lib.pfv_enc_probe_pframe_ssim_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(sizes_dev),
                                                                   ctypes.c_void_p(sse_dev), ctypes.c_void_p(ssim_q24_dev), ctypes.c_void_p(stats_dev or 0)))

    # host-buffer forms ------------------------------------------------
    def _frames(self, frames) -> np.ndarray:
        f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
        assert f.size == self.frame_bytes * self.n_streams
        return f

    def encode_iframe(self, frames) -> np.ndarray:
        """src/enc.rs:84-97 for every stream; returns coef int16 [n_streams, total_blocks, 256]."""
        f = self._frames(frames)
        coef = np.empty((self.n_streams, self.total_blocks, 256), dtype=np.int16)
        self.ctx.check(self.ctx._lib.pfv_enc_iframe(self.handle, ptr(f), ptr(coef)))
        return coef

    def encode_pframe(self, frames):
        """src/enc.rs:134-147 for every stream; returns (mv, has_coef, coef)."""
        f = self._frames(frames)
        mv = np.empty((self.n_streams, self.total_blocks, 2), dtype=np.int8)
        has = np.empty((self.n_streams, self.total_blocks), dtype=np.uint8)
        coef = np.empty((self.n_streams, self.total_blocks, 256), dtype=np.int16)
        self.ctx.check(self.ctx._lib.pfv_enc_pframe(self.handle, ptr(f), ptr(mv), ptr(has), ptr(coef)))
        return mv, has, coef

    def prev_frame(self) -> np.ndarray:
        out = np.empty((self.n_streams, self.padded_frame_bytes), dtype=np.uint8)
        self.ctx.check(self.ctx._lib.pfv_enc_prev_frame(self.handle, ptr(out)))
        return out

    # device-pointer forms (asynchronous on the context's stream) -------
    def encode_iframe_dev(self, frames_dev: int, coef_dev: int):
        self.ctx.check(self.ctx._lib.pfv_enc_iframe_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(coef_dev)))

    def encode_pframe_dev(self, frames_dev: int, mv_dev: int, has_dev: int, coef_dev: int):
        self.ctx.check(self.ctx._lib.pfv_enc_pframe_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(mv_dev),
                                                        ctypes.c_void_p(has_dev), ctypes.c_void_p(coef_dev)))

    def ingest_rgb_dev(self, pictures_dev: int, fmt="rgb8", pitch: int = 0, stride: int = 0, chroma="point") -> int:
        """asynchronous: the RGB pictures of the window's slots (slot k's at pictures_dev + k * stride, rows `pitch` apart; 0: tight) into
        slot k's frame of a packed buffer the session owns; returns that buffer's device address, a `frames_dev` for the encode, probe,
        distortion_dev and ssim_dev calls (pfv_enc_ingest_rgb_dev)"""
        from .quality import chroma_mode, pix_format
        out = ctypes.c_void_p()
        self.ctx.check(self.ctx._lib.pfv_enc_ingest_rgb_dev(self.handle, ctypes.c_void_p(pictures_dev), pix_format(fmt), int(pitch), int(stride),
                                                            chroma_mode(chroma), ctypes.byref(out)))
        return int(out.value)

    def scale_dev(self, scaler, frames_dev: int, src_stride: int = 0) -> int:
        """asynchronous: the frames of the scaler's source size of the window's slots (slot k's at frames_dev + k * src_stride; 0: packed)
        resized into slot k's frame of a packed buffer the session owns; returns that buffer's device address, a `frames_dev` for the
        encode, probe, distortion_dev and ssim_dev calls (pfv_enc_scale_dev)"""
        out = ctypes.c_void_p()
        self.ctx.check(self.ctx._lib.pfv_enc_scale_dev(self.handle, scaler.handle, ctypes.c_void_p(frames_dev), int(src_stride), ctypes.byref(out)))
        return int(out.value)

    def denoise_dev(self, denoiser, frames_dev: int, src_stride: int = 0, commit: bool = True) -> int:
        """asynchronous: the packed frames of the window's slots (slot k's at frames_dev + k * src_stride; 0: packed) through the noise filter
        as the denoiser's streams k into slot k's frame of a packed buffer the session owns; returns that buffer's device address, a
        `frames_dev` for the encode, probe, distortion_dev and ssim_dev calls (pfv_enc_denoise_dev)"""
        out = ctypes.c_void_p()
        self.ctx.check(self.ctx._lib.pfv_enc_denoise_dev(self.handle, denoiser.handle, ctypes.c_void_p(frames_dev), int(src_stride), 1 if commit else 0,
                                                         ctypes.byref(out)))
        return int(out.value)

    # GOP-batched use: the slots hold the GOPs of one stream (include/pfv_hip.h, pfv_enc_session_set_window) -----------
    def set_frame_stride(self, stride_bytes: int = 0):
        self.ctx.check(self.ctx._lib.pfv_enc_session_set_frame_stride(self.handle, int(stride_bytes)))

    def set_window(self, first: int = 0, count: int | None = None):
        count = int(self.n_streams - first if count is None else count)
        self.ctx.check(self.ctx._lib.pfv_enc_session_set_window(self.handle, int(first), count))
        self._win_count = count

    # device entropy stage (RLE + Huffman + bit packing of enc.rs:237-470 on the device) ---------------
    def enable_entropy(self, payload_cap: int = 0, async_stream: bool = False):
        """allocate the stage; payload_cap = bytes per stream (0: worst case for the geometry).  async_stream: run it
        on its own HIP stream (the caller then alternates between two sets of encode output buffers)"""
        self.ctx.check(self.ctx._lib.pfv_enc_entropy_enable(self.handle, int(payload_cap)))
        self.ctx.check(self.ctx._lib.pfv_enc_entropy_set_async(self.handle, 1 if async_stream else 0))

    def entropy_join(self):
        """the context's stream waits for the entropy stage (no host synchronisation)"""
        self.ctx.check(self.ctx._lib.pfv_enc_entropy_join(self.handle))

    def pack_iframe_dev(self, coef_dev: int):
        self.ctx.check(self.ctx._lib.pfv_enc_pack_iframe_dev(self.handle, ctypes.c_void_p(coef_dev)))

    def pack_pframe_dev(self, mv_dev: int, has_dev: int, coef_dev: int):
        self.ctx.check(self.ctx._lib.pfv_enc_pack_pframe_dev(self.handle, ctypes.c_void_p(mv_dev), ctypes.c_void_p(has_dev),
                                                             ctypes.c_void_p(coef_dev)))

    def payload_sizes(self) -> np.ndarray:
        """bytes per stream of the last pack call (synchronises); raises PfvError on oversize coefficients / capacity"""
        sizes = np.zeros(self.n_streams, dtype=np.uint32)
        self.ctx.check(self.ctx._lib.pfv_enc_payload_sizes(self.handle, ptr(sizes)))
        return sizes

    def payload(self, stream: int, nbytes: int) -> bytes:
        out = np.empty(max(int(nbytes), 1), dtype=np.uint8)
        self.ctx.check(self.ctx._lib.pfv_enc_payload_fetch(self.handle, int(stream), ptr(out), int(nbytes)))
        return out[:nbytes].tobytes()

    def payloads(self, out: np.ndarray):
        """all streams' payloads of the last pack call with one device-to-host copy into `out` (uint8, ideally from
        Context.host_array); returns (sizes, offsets): stream s is out[offsets[s] : offsets[s] + sizes[s]]"""
        sizes = np.zeros(self.n_streams, dtype=np.uint32)
        offsets = np.zeros(self.n_streams, dtype=np.uint64)
        self.ctx.check(self.ctx._lib.pfv_enc_payloads_fetch(self.handle, ptr(out), out.size, ptr(sizes), ptr(offsets)))
        return sizes, offsets

    def payload_dev(self, stream: int) -> int:
        return int(self.ctx._lib.pfv_enc_payload_dev(self.handle, int(stream)) or 0)

    # distortion: the frames just encoded against the current prev_frame (pfv_enc_distortion_dev) ---------------
    def distortion_dev(self, frames_dev: int, sse_dev: int, mb_sse_dev: int = 0):
        """asynchronous on the context's stream; sse_dev uint64 [n_streams][3], mb_sse_dev uint32 [n_streams][total_blocks] or 0 (the
        map then stays in the session's scratch).  Honours the window and the frame stride."""
        self.ctx.check(self.ctx._lib.pfv_enc_distortion_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(sse_dev),
                                                            ctypes.c_void_p(mb_sse_dev or 0)))

    def distortion(self, frames, mb_map: bool = False, out=None, out_map=None):
        """squared error per plane, uint64 [n_streams, 3], between `frames` -- the frames handed to the last encode call, as an array
        (uploaded as it is: with a frame stride set it holds the strided layout) or a device address -- and what a decoder will show for
        them; with mb_map also the per-macroblock map uint32 [n_streams, total_blocks].  Entries of slots outside the window keep the
        values of `out` / `out_map` (zeros when not given)."""
        from .quality import session_distortion
        return session_distortion(self, self.distortion_dev, frames, mb_map, out, out_map)

    # structural similarity of the same pair of frames (pfv_enc_ssim_dev) ---------------
    def ssim_dev(self, frames_dev: int, ssim_q24_dev: int, mb_dev: int = 0):
        """asynchronous on the context's stream; ssim_q24_dev int64 [n_streams][3], mb_dev int32 [n_streams][total_blocks] or 0 (the map
        then stays in the session's scratch).  Operands, window and stride as distortion_dev."""
        self.ctx.check(self.ctx._lib.pfv_enc_ssim_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(ssim_q24_dev),
                                                      ctypes.c_void_p(mb_dev or 0)))

    def ssim(self, frames, mb_map: bool = False, out=None, out_map=None):
        """SSIM sums per plane in 2^-24 fixed point, int64 [n_streams, 3] (quality.ssim / quality.ssim_windows give the mean); with mb_map
        also the per-macroblock map int32 [n_streams, total_blocks].  Arguments as distortion."""
        from .quality import session_distortion
        return session_distortion(self, self.ssim_dev, frames, mb_map, out, out_map, sum_dtype=np.int64, map_dtype=np.int32)


class DecoderSession(_Geometry):
    def __init__(self, ctx: Context, width: int, height: int, qtables, n_streams: int = 1):
        super().__init__(width, height, n_streams)
        self.ctx = ctx
        q = np.ascontiguousarray(qtables, dtype=np.int32).reshape(-1, 64)
        h = ctypes.c_void_p()
        ctx.check(ctx._lib.pfv_dec_session_create(ctx.handle, int(width), int(height), ptr(q), int(q.shape[0]),
                                                  int(n_streams), ctypes.byref(h)))
        self.handle = h
        ctx._sessions.add(self)

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            self.ctx._lib.pfv_dec_session_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _qidx(qidx) -> np.ndarray:
        q = np.ascontiguousarray(qidx, dtype=np.uint8)
        assert q.shape == (3,)
        return q

    def decode_iframe(self, coef, qidx=(0, 1, 1)):
        c = np.ascontiguousarray(coef, dtype=np.int16)
        assert c.size == self.n_streams * self.total_blocks * 256
        self.ctx.check(self.ctx._lib.pfv_dec_iframe(self.handle, ptr(c), ptr(self._qidx(qidx))))

    def decode_iframe_sparse(self, idx, val, qidx=(0, 1, 1)):
        """non-zero coefficients as (flat index into [stream][macroblock][256], value) pairs; the rest is zero"""
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        v = np.ascontiguousarray(val, dtype=np.int16)
        assert i.shape == v.shape and i.ndim == 1
        self.ctx.check(self.ctx._lib.pfv_dec_iframe_sparse(self.handle, ptr(i), ptr(v), i.size, ptr(self._qidx(qidx))))

    def decode_pframe_sparse(self, mv, has_coef, idx, val, qidx=(2, 3, 3)):
        m = np.ascontiguousarray(mv, dtype=np.int8)
        hc = np.ascontiguousarray(has_coef, dtype=np.uint8)
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        v = np.ascontiguousarray(val, dtype=np.int16)
        assert i.shape == v.shape and i.ndim == 1
        self.ctx.check(self.ctx._lib.pfv_dec_pframe_sparse(self.handle, ptr(m), ptr(hc), ptr(i), ptr(v), i.size, ptr(self._qidx(qidx))))

    def decode_pframe(self, mv, has_coef, coef, qidx=(2, 3, 3)):
        m = np.ascontiguousarray(mv, dtype=np.int8)
        hc = np.ascontiguousarray(has_coef, dtype=np.uint8)
        c = np.ascontiguousarray(coef, dtype=np.int16)
        assert c.size == self.n_streams * self.total_blocks * 256
        self.ctx.check(self.ctx._lib.pfv_dec_pframe(self.handle, ptr(m), ptr(hc), ptr(c), ptr(self._qidx(qidx))))

    def coef_lists(self, coef, has_coef=None):
        """dense coefficients [n_streams][total_blocks][256] -> (entries per stream, counts [n_streams][total_blocks + 1]): the
        coefficient-list form of pfv_dec_*_lists_dev (pfv_coef_lists_from_dense)"""
        c = np.ascontiguousarray(coef, dtype=np.int16).reshape(self.n_streams, self.total_blocks * 256)
        hc = None if has_coef is None else np.ascontiguousarray(has_coef, dtype=np.uint8).reshape(self.n_streams, self.total_blocks)
        entries, counts = [], np.zeros((self.n_streams, self.total_blocks + 1), dtype=np.uint32)
        for k in range(self.n_streams):
            e = np.empty(self.total_blocks * 256, dtype=np.uint32)
            n = ctypes.c_size_t(0)
            rc = self.ctx._lib.pfv_coef_lists_from_dense(ptr(c[k]), ptr(hc[k]) if hc is not None else None, self.total_blocks, ptr(e), e.size,
                                                         ptr(counts[k]), ctypes.byref(n))
            assert rc == 0, rc
            entries.append(e[:n.value].copy())
        return entries, counts

    def _upload_lists(self, entries, counts):
        """entries of all slots back to back in one device buffer + the table of list pointers + the counts; returns the three device
        addresses (the caller frees them)"""
        ctx = self.ctx
        sizes = [max(int(e.size), 1) for e in entries]
        ent_dev = ctx.alloc(4 * sum(sizes))
        ptrs = np.zeros(self.n_streams, dtype=np.uint64)
        off = 0
        for k, e in enumerate(entries):
            ptrs[k] = ent_dev + 4 * off
            if e.size:
                ctx.upload(ent_dev + 4 * off, np.ascontiguousarray(e, dtype=np.uint32))
            off += sizes[k]
        ptr_dev = ctx.alloc(8 * self.n_streams)
        ctx.upload(ptr_dev, ptrs)
        r = np.ascontiguousarray(counts, dtype=np.uint32)
        rng_dev = ctx.alloc(r.nbytes)
        ctx.upload(rng_dev, r)
        return ent_dev, ptr_dev, rng_dev

    def decode_iframe_lists(self, entries, counts, qidx=(0, 1, 1)):
        """i-frame from coefficient lists (coef_lists): same framebuffer as decode_iframe on the dense array"""
        bufs = self._upload_lists(entries, counts)
        try:
            self.ctx.check(self.ctx._lib.pfv_dec_iframe_lists_dev(self.handle, ctypes.c_void_p(bufs[1]), ctypes.c_void_p(bufs[2]), ptr(self._qidx(qidx))))
            self.ctx.sync()
        finally:
            for b in bufs:
                self.ctx.free(b)

    def decode_pframe_lists(self, mv, has_coef, entries, counts, qidx=(2, 3, 3)):
        ctx = self.ctx
        m = np.ascontiguousarray(mv, dtype=np.int8)
        hc = np.ascontiguousarray(has_coef, dtype=np.uint8)
        bufs = list(self._upload_lists(entries, counts))
        try:
            mv_dev = ctx.alloc(m.nbytes); bufs.append(mv_dev)
            has_dev = ctx.alloc(hc.nbytes); bufs.append(has_dev)
            ctx.upload(mv_dev, m)
            ctx.upload(has_dev, hc)
            ctx.check(ctx._lib.pfv_dec_pframe_lists_dev(self.handle, ctypes.c_void_p(mv_dev), ctypes.c_void_p(has_dev), ctypes.c_void_p(bufs[1]),
                                                        ctypes.c_void_p(bufs[2]), ptr(self._qidx(qidx))))
            self.check()
        finally:
            for b in bufs:
                ctx.free(b)

    def decode_iframe_dev(self, coef_dev: int, qidx=(0, 1, 1)):
        self.ctx.check(self.ctx._lib.pfv_dec_iframe_dev(self.handle, ctypes.c_void_p(coef_dev), ptr(self._qidx(qidx))))

    def decode_pframe_dev(self, mv_dev: int, has_dev: int, coef_dev: int, qidx=(2, 3, 3)):
        self.ctx.check(self.ctx._lib.pfv_dec_pframe_dev(self.handle, ctypes.c_void_p(mv_dev), ctypes.c_void_p(has_dev),
                                                        ctypes.c_void_p(coef_dev), ptr(self._qidx(qidx))))

    def check(self):
        self.ctx.check(self.ctx._lib.pfv_dec_check(self.handle))

    def enable_path_stats(self, on: bool = True):
        """count the wavefronts whose inverse transform ran in i32 because their values failed the float guard, from zero
        (pfv_dec_session_enable_path_stats; PFV_OPT_DEC_TRANSFORM)"""
        self.ctx.check(self.ctx._lib.pfv_dec_session_enable_path_stats(self.handle, 1 if on else 0))

    def path_stats(self):
        """(integer-path wavefronts, wavefronts launched) since enable_path_stats (pfv_dec_session_path_stats)"""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        self.ctx.check(self.ctx._lib.pfv_dec_session_path_stats(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def get_frame(self) -> np.ndarray:
        """retframe of every stream (src/dec.rs:195-197): uint8 [n_streams, frame_bytes]."""
        out = np.empty((self.n_streams, self.frame_bytes), dtype=np.uint8)
        self.ctx.check(self.ctx._lib.pfv_dec_get_frame(self.handle, ptr(out)))
        return out

    def set_output_dev(self, frames_dev):
        """fuse the retframe crop into the decode kernels (None switches it off)"""
        self.ctx.check(self.ctx._lib.pfv_dec_set_output_dev(self.handle, ctypes.c_void_p(frames_dev or 0)))

    def set_output_strided_dev(self, frames_dev, stride_bytes: int):
        """retframes of consecutive slots `stride_bytes` apart (GOP-batched decode: the stream appears in display order)"""
        self.ctx.check(self.ctx._lib.pfv_dec_set_output_strided_dev(self.handle, ctypes.c_void_p(frames_dev or 0), int(stride_bytes)))

    def set_window(self, first: int = 0, count: int | None = None):
        self.ctx.check(self.ctx._lib.pfv_dec_session_set_window(self.handle, int(first), int(self.n_streams - first if count is None else count)))

    def get_frame_dev(self, frames_dev: int):
        self.ctx.check(self.ctx._lib.pfv_dec_get_frame_dev(self.handle, ctypes.c_void_p(frames_dev)))

    def set_deblock(self, mode=None, strength=None):
        """out-of-loop deblocking of every frame that leaves the session (get_frame, get_frame_dev, the output buffer): "off", "auto"
        (strengths from the q-tables the last decode call named) or "fixed" with strength = (Y, U, V), each 0..12.  The framebuffer and
        what the next p-frame predicts from are untouched (pfv_dec_set_deblock)."""
        from .quality import deblock_args
        m, p, _keep = deblock_args(mode, strength)
        self.ctx.check(self.ctx._lib.pfv_dec_set_deblock(self.handle, m, p))

    # RGB / RGBA / BGRA pictures of what get_frame would return (k_present_rgb) ---------------
    def get_frame_rgb(self, fmt="rgb8") -> np.ndarray:
        """every stream's picture, tight: uint8 [n_streams, height, width, 3 or 4]; fmt "rgb8" / "rgba8" / "bgra8" (pfv_dec_get_frame_rgb)"""
        from .quality import pix_format, rgb_shape
        m = pix_format(fmt)
        out = np.empty((self.n_streams,) + rgb_shape(self.ctx, self.width, self.height, m), dtype=np.uint8)
        self.ctx.check(self.ctx._lib.pfv_dec_get_frame_rgb(self.handle, ptr(out), m))
        return out

    def get_frame_rgb_dev(self, dst_dev: int, fmt="rgb8", pitch: int = 0, stride: int = 0):
        """asynchronous; rows `pitch` bytes apart (0: tight), pictures `stride` apart (0: pitch x height) (pfv_dec_get_frame_rgb_dev)"""
        from .quality import pix_format
        self.ctx.check(self.ctx._lib.pfv_dec_get_frame_rgb_dev(self.handle, ctypes.c_void_p(dst_dev), pix_format(fmt), int(pitch), int(stride)))

    def set_output_scaled_dev(self, scaler, dst_dev, stride: int = 0):
        """a resized output beside the others: every decode call also writes the frames of its window's slots at the scaler's destination
        size, packed, `stride` apart (0: the frame size), indexed by slot; dst_dev None switches it off.  The scaler must stay open while
        it is set (pfv_dec_set_output_scaled_dev)"""
        self._scaled_keep = scaler if dst_dev else None
        self.ctx.check(self.ctx._lib.pfv_dec_set_output_scaled_dev(self.handle, scaler.handle if (scaler is not None and dst_dev) else None,
                                                                  ctypes.c_void_p(dst_dev or 0), int(stride)))

    def set_output_rgb_dev(self, dst_dev, fmt="rgb8", pitch: int = 0, stride: int = 0):
        """an RGB output beside the planar ones: every decode call also writes the pictures of its window's slots, indexed by slot
        (None switches it off) (pfv_dec_set_output_rgb_dev)"""
        from .quality import pix_format
        self.ctx.check(self.ctx._lib.pfv_dec_set_output_rgb_dev(self.handle, ctypes.c_void_p(dst_dev or 0), pix_format(fmt), int(pitch), int(stride)))

    def framebuffer(self) -> np.ndarray:
        out = np.empty((self.n_streams, self.padded_frame_bytes), dtype=np.uint8)
        self.ctx.check(self.ctx._lib.pfv_dec_framebuffer(self.handle, ptr(out)))
        return out

    # distortion: packed frames against the current framebuffer (pfv_dec_distortion_dev) ---------------
    def distortion_dev(self, frames_dev: int, sse_dev: int, mb_sse_dev: int = 0):
        self.ctx.check(self.ctx._lib.pfv_dec_distortion_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(sse_dev),
                                                            ctypes.c_void_p(mb_sse_dev or 0)))

    def distortion(self, frames, mb_map: bool = False, out=None, out_map=None):
        """squared error per plane, uint64 [n_streams, 3], between `frames` (packed originals: an array or a device address) and the
        decoded frames; see EncoderSession.distortion"""
        from .quality import session_distortion
        return session_distortion(self, self.distortion_dev, frames, mb_map, out, out_map)

    # structural similarity of the same pair of frames (pfv_dec_ssim_dev) ---------------
    def ssim_dev(self, frames_dev: int, ssim_q24_dev: int, mb_dev: int = 0):
        """asynchronous on the context's stream; ssim_q24_dev int64 [n_streams][3], mb_dev int32 [n_streams][total_blocks] or 0 (the map
        then stays in the session's scratch).  Operands, window and stride as distortion_dev."""
        self.ctx.check(self.ctx._lib.pfv_dec_ssim_dev(self.handle, ctypes.c_void_p(frames_dev), ctypes.c_void_p(ssim_q24_dev),
                                                      ctypes.c_void_p(mb_dev or 0)))

    def ssim(self, frames, mb_map: bool = False, out=None, out_map=None):
        """SSIM sums per plane in 2^-24 fixed point, int64 [n_streams, 3] (quality.ssim / quality.ssim_windows give the mean); with mb_map
        also the per-macroblock map int32 [n_streams, total_blocks].  Arguments as distortion."""
        from .quality import session_distortion
        return session_distortion(self, self.ssim_dev, frames, mb_map, out, out_map, sum_dtype=np.int64, map_dtype=np.int32)
