// pfv_container.hip -- the .pfv container, host code only: magic and version (src/common.rs:1-2), the header (src/enc.rs:190-219,
// src/dec.rs:38-134), the 5-byte packet head and the EOF marker (src/enc.rs:221-235), one step of the packet loop (src/dec.rs:174-222).
// The stream objects write and read the container through this file alone.
// Part of the one translation unit of the C ABI: included by pfv_capi.hip, in this order, never compiled on its own.
static const uint8_t kPfvMagic[8] = {'P', 'F', 'V', 'I', 'D', 'E', 'O', 0};   // common.rs:1
constexpr uint32_t kPfvVersion = 211;                                           // common.rs:2: codec 2.1.1
static const uint8_t kPfvEof[5] = {0, 0, 0, 0, 0};                              // the EOF marker: a packet head of type 0 and length 0 (enc.rs:221-227)

static void put_u16(std::vector<uint8_t> &o, unsigned v) { o.push_back((uint8_t)v); o.push_back((uint8_t)(v >> 8)); }
static void put_u32(std::vector<uint8_t> &o, uint32_t v) { for (int i = 0; i < 4; i++) o.push_back((uint8_t)(v >> (8 * i))); }
static inline int get_u16(const uint8_t *p) { return (int)p[0] | ((int)p[1] << 8); }
static inline uint32_t get_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// packet head (enc.rs:301-305, :453-457): the type, then the payload's length
static inline void put_packet_head(uint8_t h[5], uint8_t type, uint32_t plen)
{
    h[0] = type; h[1] = (uint8_t)plen; h[2] = (uint8_t)(plen >> 8); h[3] = (uint8_t)(plen >> 16); h[4] = (uint8_t)(plen >> 24);
}
static void put_packet(std::vector<uint8_t> &o, uint8_t type, const uint8_t *payload, size_t plen)
{
    uint8_t h[5];
    put_packet_head(h, type, (uint32_t)plen);
    o.insert(o.end(), h, h + 5);
    if (plen) o.insert(o.end(), payload, payload + plen);
}

// write_header (enc.rs:190-219) for a ladder of qualities: 4 * n_rungs tables, rung-major, each rung in the order intra_l, intra_c, inter_l,
// inter_c
static void put_header(std::vector<uint8_t> &o, int width, int height, int framerate, const int *qualities, int n_rungs)
{
    o.insert(o.end(), kPfvMagic, kPfvMagic + 8);
    put_u32(o, kPfvVersion);
    put_u16(o, (unsigned)width); put_u16(o, (unsigned)height); put_u16(o, (unsigned)framerate);
    put_u16(o, 4u * (unsigned)n_rungs);
    for (int r = 0; r < n_rungs; r++) {
        int32_t q[4][64];
        pfv_qtables_from_quality(qualities[r], q[0], q[1], q[2], q[3], nullptr);
        for (int t = 0; t < 4; t++)
            for (int i = 0; i < 64; i++) put_u16(o, (unsigned)q[t][i]);
    }
}

// Decoder::new's read of the header (dec.rs:38-134), in the reference's order: magic, version, geometry, frame rate, table count, tables.
struct PfvHeader {
    int width = 0, height = 0, framerate = 0, n_qtables = 0;
    std::vector<int32_t> q;      // [max(n_qtables, 1)][64]: a stream without tables opens (its packets cannot name one)
    size_t len = 0;              // bytes of the header: where the first packet starts
};
static int read_header(pfv_ctx *ctx, const uint8_t *data, size_t len, PfvHeader &h)
{
    if (len < 8) return fail(ctx, PFV_ERR_IO, "stream shorter than the magic (DecodeError::IOError)");
    if (memcmp(data, kPfvMagic, 8) != 0) return fail(ctx, PFV_ERR_FORMAT, "bad magic (DecodeError::FormatError, src/dec.rs:50-52)");
    if (len < 12) return fail(ctx, PFV_ERR_IO, "truncated header");
    if (get_u32(data + 8) != kPfvVersion) return fail(ctx, PFV_ERR_VERSION, "codec version is not 2.1.1 (DecodeError::VersionError, src/dec.rs:57-59)");
    if (len < 20) return fail(ctx, PFV_ERR_IO, "truncated header");
    h.width = get_u16(data + 12); h.height = get_u16(data + 14); h.framerate = get_u16(data + 16); h.n_qtables = get_u16(data + 18);
    h.len = 20 + (size_t)h.n_qtables * 128;
    if (len < h.len) return fail(ctx, PFV_ERR_IO, "truncated q-tables");
    h.q.assign((size_t)std::max(h.n_qtables, 1) * 64, 1);
    for (size_t i = 0; i < (size_t)h.n_qtables * 64; i++) h.q[i] = get_u16(data + 20 + 2 * i);
    return PFV_OK;
}

// One step of the reference's packet loop (dec.rs:174-222): the packet at `pos`.  PFV_OK: its type, payload and the position behind it -- for
// the EOF marker (type 0) behind its head, whatever length that names.  PFV_ERR_IO with `msg`: the stream ends inside the head (pos_after =
// pos) or inside the payload (pos_after = behind the head), where the reference's reader stands after the failed read.  What a type means
// is the caller's business.
struct PfvPacket {
    uint8_t type = 0;
    const uint8_t *payload = nullptr;
    uint32_t plen = 0;
    size_t pos_after = 0;
    const char *msg = "";
};
static int next_packet(const uint8_t *data, size_t len, size_t pos, PfvPacket &p)
{
    p = PfvPacket();
    p.pos_after = pos;
    if (pos + 5 > len) { p.msg = "unexpected end of stream in a packet header"; return PFV_ERR_IO; }
    p.type = data[pos];
    p.pos_after = pos += 5;
    if (p.type == 0) return PFV_OK;   // EOF marker (:183-187)
    p.plen = get_u32(data + pos - 4);
    if (pos + p.plen > len) { p.msg = "packet payload runs past the end of the stream"; return PFV_ERR_IO; }
    p.payload = data + pos;
    p.pos_after = pos + p.plen;
    return PFV_OK;
}
