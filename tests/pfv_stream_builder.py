""".pfv streams written from parts (src/enc.rs:190-235, src/dec.rs:38-224): a header with ANY set of q-tables, packets whose payloads the
oracle's serialisers write (oracle/pfv_oracle_entropy.c) with the three per-plane q-table indices of payload bytes 16-18 set to whatever the
test chooses, drop frames and the EOF packet.  The product's encoders only ever write (0,1,1) / (2,3,3) and four tables; the decoders must
take any choice the format allows."""
from __future__ import annotations

import ctypes

import numpy as np

from parity_cases import _oracle_serializers

MAGIC = b"PFVIDEO\0"
VERSION = 211
ENCODER_QIDX = {1: (0, 1, 1), 2: (2, 3, 3)}        # what write_iframe_packet / write_pframe_packet put there (src/enc.rs:296-298, 409-411)
MAX_COEF = 16383                                   # a 16-bit size class panics in the reference (rle.rs:44)


def header(w, h, fps, tables) -> bytes:
    """magic, version, w, h, fps, num_qtable (u16), then the tables as u16 (src/enc.rs:199-215); tables: [n, 64] ints in [0, 65535]"""
    t = np.asarray(tables, dtype=np.int64).reshape(-1, 64)
    assert t.shape[0] <= 65535 and (t.size == 0 or (t.min() >= 0 and t.max() <= 65535))
    head = MAGIC + VERSION.to_bytes(4, "little") + b"".join(int(v).to_bytes(2, "little") for v in (w, h, fps, t.shape[0]))
    return head + t.astype("<u2").tobytes()


class StreamBuilder:
    """one .pfv stream: add packets in order, bytes() appends the EOF packet"""

    def __init__(self, oracle, w, h, fps, tables, total_blocks):
        self.L = _oracle_serializers(oracle)
        self.nb = int(total_blocks)
        self.parts = [header(w, h, fps, tables)]
        self.kinds = []                              # 'I' / 'P' / 'D' per packet
        self._buf = np.zeros(self.nb * 256 * 4 + 4096, np.uint8)     # worst case: every coefficient 15 size bits + codes

    def _payload(self, n, ptype, qidx):
        pay = bytearray(self._buf[:n].tobytes())
        assert tuple(pay[16:19]) == ENCODER_QIDX[ptype], "the serialiser no longer writes the q-table indices at payload bytes 16-18"
        assert all(0 <= int(q) <= 255 for q in qidx)
        pay[16:19] = bytes(int(q) for q in qidx)
        return bytes(pay)

    def _packet(self, ptype, payload):
        self.parts.append(bytes([ptype]) + len(payload).to_bytes(4, "little") + payload)

    def iframe(self, coef, qidx):
        c = np.ascontiguousarray(coef, dtype=np.int16).reshape(self.nb, 256)
        assert np.abs(c.astype(np.int32)).max(initial=0) <= MAX_COEF
        n = self.L.pfvo_serialize_iframe(c.ctypes.data_as(ctypes.c_void_p), self.nb, self._buf.ctypes.data_as(ctypes.c_void_p), self._buf.size)
        assert 19 <= n <= self._buf.size
        self._packet(1, self._payload(n, 1, qidx))
        self.kinds.append("I")

    def pframe(self, mv, has, coef, qidx):
        m = np.ascontiguousarray(mv, dtype=np.int8).reshape(self.nb, 2)
        hc = np.ascontiguousarray(has, dtype=np.uint8).reshape(self.nb)
        c = np.ascontiguousarray(coef, dtype=np.int16).reshape(self.nb, 256)
        assert np.abs(c.astype(np.int32)).max(initial=0) <= MAX_COEF
        n = self.L.pfvo_serialize_pframe(m.ctypes.data_as(ctypes.c_void_p), hc.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p),
                                         self.nb, self._buf.ctypes.data_as(ctypes.c_void_p), self._buf.size)
        assert 19 <= n <= self._buf.size
        self._packet(2, self._payload(n, 2, qidx))
        self.kinds.append("P")

    def drop(self):
        self._packet(1, b"")                          # a type-1 packet of length 0 (src/dec.rs:188-202)
        self.kinds.append("D")

    def bytes(self) -> bytes:
        return b"".join(self.parts) + bytes(5)        # EOF: type 0, length 0 (src/enc.rs:221-227)
