// TCP receive placement over pool buffers (rns_rx_tcp_place_pool_dev): tcp_input's decode, the
// PORT_MAP lookup and tcp_read's copy, for datagrams the pool receive verify has judged.
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_pool_rx.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// The entry point runs rx_pool_kernel as it is (d_status / d_l4_sum are rns_rx_verify_pool_dev's by
// construction, and its instantiations keep their instructions) and then this kernel on the same
// stream, which reads the statuses back.  A wave owns one 64-datagram block, the unit of
// d_blk_first, so a lane's first fragment is d_blk_first[block] + the DPP prefix sum of the
// block's fragment counts, as in the verify.
//
// Decode and lookup, one datagram per lane.  An accepted datagram's IP header and the fixed 20
// TCP bytes (at most 60 + 20) lie in its first buffer (B >= 128), 4-byte aligned, and inside the
// datagram once L >= 20: the lane reads them as dwords where they lie — its first dword for the
// header length, the TCP header's five, the source address — a few lines the verify has just
// pulled through L2.  The flow table is an open-addressed hash of 32-byte slots built by
// rns_rx_flow_table_build (k_place.hip); a probe ends at an empty slot or after `slots` steps,
// and a stored flow index >= n_flows never matches, so any table bytes are safe to read.
//
// Placement, the whole wave on its placed datagrams together.  Every destination range is cut into
// its 16-byte-aligned chunks and the wave walks the chunks of all its datagrams concatenated (the
// prefix sum of the chunk counts in LDS, a six-step search per chunk), 128 at a time with both
// halves' loads in flight, so short payloads fill the lanes as well as long ones.  A destination
// chunk draws on the two aligned source chunks around the same payload bytes (each inside one
// buffer, B a multiple of 16: one index load per chunk), joined at the byte shift (source offset -
// destination address) & 15, which is the same for every chunk of a datagram; the second of the two
// is the next destination chunk's first, so a lane takes it from the next lane where that lane holds
// the same datagram and loads it only at a datagram's or the wave's edge.  Whole chunks go out
// as one aligned 16-byte store; the first and last chunk of a payload, where not whole, as byte
// stores, so that two segments that meet inside a 16-byte granule never write each other's bytes.
// A source chunk that is not whole inside the pool (the tail of a pool whose size is no multiple
// of 16) is read byte by byte.
// ---------------------------------------------------------------------------
constexpr uint32_t kPlaceMinLog2 = 7;  // 60 + 60 header bytes lie inside the first buffer
static_assert((1u << kPlaceMinLog2) >= 60u + 60u, "IP and TCP headers lie inside the first buffer");

constexpr uint32_t kFlowSlotBytes = 32, kFlowSlotWords = 8, kFlowMinSlots = 64;

struct PlaceArgs {
    const uint8_t *pool;  // 16-byte aligned
    uint64_t pool_bytes;
    const uint32_t *buf_idx;
    const uint32_t *blk_first;
    const uint16_t *len16;
    const uint8_t *status;  // the verify's verdicts
    const uint32_t *tbl;    // the flow table's slots
    const uint32_t *next_seq;
    const uint64_t *win_off;
    const uint32_t *win_len;
    uint8_t *stream;
    uint64_t stream_bytes;
    uint32_t *meta;  // 6 dwords per datagram
    uint32_t n, n_frags, n_flows, slots, blog;
};

// Slots of the table for n_flows keys: a power of two >= 2 * n_flows and >= 64.
__host__ __device__ inline uint64_t flow_slots(uint32_t n_flows)
{
    uint64_t s = kFlowMinSlots;
    while (s < 2ull * n_flows)
        s <<= 1;
    return s;
}

// The key as six dwords: ip[0..16) as it lies in memory, sport | dport << 16, family.
__host__ __device__ inline uint32_t flow_hash(const uint32_t (&k)[6])
{
    uint32_t h = 0x9e3779b9u;
    for (int i = 0; i < 6; ++i) {
        h = (h ^ k[i]) * 0x85ebca6bu;
        h ^= h >> 15;
    }
    return h;
}

__device__ __forceinline__ uint32_t flow_lookup(const PlaceArgs &a, const uint32_t (&k)[6])
{
    const uint32_t smask = a.slots - 1u;
    uint32_t s = flow_hash(k) & smask;
    for (uint32_t t = 0; t < a.slots; ++t) {
        const uint32_t *e = a.tbl + static_cast<uint64_t>(s) * kFlowSlotWords;
        const uint32_t used = e[7];
        if (used == 0)
            break;
        if (used == 1 && e[0] == k[0] && e[1] == k[1] && e[2] == k[2] && e[3] == k[3] && e[4] == k[4] && e[5] == k[5] &&
            e[6] < a.n_flows)
            return e[6];
        s = (s + 1u) & smask;
    }
    return RNS_RX_NO_FLOW;
}

// The aligned 16-byte chunk at byte s of the datagram whose fragments start at d_buf_idx[gi]
// (s below the datagram's length, so the fragment exists); bytes outside the pool read as zero.
template <bool NT>
__device__ __forceinline__ uint4 place_load(const PlaceArgs &a, uint64_t gi, uint32_t s)
{
    const uint32_t bmask = (1u << a.blog) - 1u;
    const uint64_t at = (static_cast<uint64_t>(a.buf_idx[gi + (s >> a.blog)]) << a.blog) + (s & bmask);
    if (at <= a.pool_bytes && a.pool_bytes - at >= 16u) {
        const u32x4 *p = reinterpret_cast<const u32x4 *>(a.pool + at);
        const u32x4 v = NT ? __builtin_nontemporal_load(p) : *p;
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if (at + b < a.pool_bytes)
            w[b >> 2] |= static_cast<uint32_t>(a.pool[at + b]) << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// Per placed datagram in LDS: [0] the wave's destination chunks before it, [1] [2] its first
// fragment's place in d_buf_idx, [3] ip_hdr + tcp_hdr, [4] pay_len, [5] [6] its place in d_stream.
constexpr int kPlacePd = 7;

// One destination chunk: the first of the two source chunks around its bytes, and where they go.
struct PlaceChunk {
    uint4 x;
    uint64_t gi;        // its datagram's first fragment
    uint8_t *dc;        // the chunk's 16-byte-aligned address
    uint32_t lo, hi;    // its payload bytes are [lo, hi); hi == 0: no chunk
    uint32_t sh;        // (source offset - destination address) & 15
    uint32_t s2;        // the second source chunk's offset in the datagram, 0: not needed
    uint32_t j;         // its datagram's lane, ~0: no chunk
};

// The datagram that owns chunk v of the wave's concatenated destination chunks (row 0 of the wave's
// LDS table: the chunks before each datagram): the last one whose chunks start at or before v.
// (Shared with the echo build, rns_k_echo.hpp.)
template <int ROWS>
__device__ __forceinline__ uint32_t place_owner(const uint32_t (&pd)[ROWS][64], uint32_t v)
{
    uint32_t j = 0;
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1)
        j += pd[0][j + step] <= v ? step : 0u;
    return j;
}

// Chunk v of the wave's concatenated destination chunks, its first load issued.
template <bool NT>
__device__ __forceinline__ PlaceChunk place_fetch(const PlaceArgs &a, const uint32_t (&pd)[kPlacePd][64], uint32_t v,
                                                  uint32_t W)
{
    PlaceChunk ck{};
    ck.j = ~0u;
    if (v >= W)
        return ck;
    const uint32_t j = place_owner(pd, v);
    const uint32_t c = v - pd[0][j], skip = pd[3][j], plen = pd[4][j];
    const uint64_t gi = (static_cast<uint64_t>(pd[2][j]) << 32) | pd[1][j];
    uint8_t *const d0 = a.stream + ((static_cast<uint64_t>(pd[6][j]) << 32) | pd[5][j]);
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(d0) & 15u);
    const uint32_t T = skip + plen;                     // <= 65535
    const uint32_t o0 = skip - mis + 16u * c;           // skip >= 24 (an IP header and 20 TCP bytes)
    const uint32_t s = o0 & ~15u;
    ck.sh = o0 & 15u;
    ck.x = place_load<NT>(a, gi, s);
    ck.s2 = (ck.sh && s + 16u < T) ? s + 16u : 0u;
    ck.gi = gi;
    ck.j = j;
    ck.dc = d0 - mis + 16ull * c;
    ck.lo = c == 0 ? mis : 0u;
    ck.hi = min(16u, mis + plen - 16u * c);             // >= 1: c is below the datagram's chunk count
    return ck;
}

// The second source chunk.  The next lane's chunk, when it is the same datagram's, is the next
// destination chunk, whose first source chunk is this one's second: taken from that lane instead of
// memory.  (Called by the whole wave.)
template <bool NT>
__device__ __forceinline__ uint4 place_second(const PlaceArgs &a, const PlaceChunk &ck, uint32_t lane)
{
    const uint32_t jn = static_cast<uint32_t>(__shfl_down(static_cast<int>(ck.j), 1, 64));
    uint4 y = make_uint4(static_cast<uint32_t>(__shfl_down(static_cast<int>(ck.x.x), 1, 64)),
                         static_cast<uint32_t>(__shfl_down(static_cast<int>(ck.x.y), 1, 64)),
                         static_cast<uint32_t>(__shfl_down(static_cast<int>(ck.x.z), 1, 64)),
                         static_cast<uint32_t>(__shfl_down(static_cast<int>(ck.x.w), 1, 64)));
    if (ck.s2 == 0)
        y = make_uint4(0u, 0u, 0u, 0u);
    else if (lane == 63u || jn != ck.j)
        y = place_load<NT>(a, ck.gi, ck.s2);
    return y;
}

// The destination chunk's 16 bytes: the two source chunks joined at the byte shift.
__device__ __forceinline__ void place_join(const PlaceChunk &ck, const uint4 y, uint32_t (&o)[4])
{
    const uint32_t q = ck.sh >> 2, bs = ck.sh & 3u;
    const uint32_t w[8] = {ck.x.x, ck.x.y, ck.x.z, ck.x.w, y.x, y.y, y.z, y.w};
    uint32_t d[5];
#pragma unroll
    for (int k = 0; k < 5; ++k)
        d[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        o[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], bs);
}

__device__ __forceinline__ void place_emit(const PlaceChunk &ck, const uint4 y)
{
    if (ck.hi == 0)
        return;
    uint32_t o[4];
    place_join(ck, y, o);
    if (ck.lo == 0 && ck.hi == 16u) {
        *reinterpret_cast<uint4 *>(ck.dc) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int b = 0; b < 16; ++b)
            if (static_cast<uint32_t>(b) >= ck.lo && static_cast<uint32_t>(b) < ck.hi)
                ck.dc[b] = static_cast<uint8_t>(o[b >> 2] >> (8 * (b & 3)));
    }
}

// A datagram's place in the pool form, as the verify and the placement compute it (whole wave).
// (Shared by the echo responder and the UDP demux, rns_k_echo.hpp and rns_k_udp.hpp.)
struct PoolLane {
    uint64_t p, gi;
    uint32_t T, nf;
    bool live;
};

__device__ __forceinline__ PoolLane pool_lane(const PlaceArgs &a, uint32_t blk, uint32_t lane)
{
    PoolLane e;
    e.p = static_cast<uint64_t>(blk) * 64 + lane;
    e.live = e.p < a.n;
    const uint32_t bmask = (1u << a.blog) - 1u;
    e.T = e.live ? a.len16[e.p] : 0u;
    e.nf = (e.T + bmask) >> a.blog;
    const uint32_t inc = wave_incl_scan(e.nf);
    const uint32_t first = static_cast<uint64_t>(blk) * 64 < a.n ? a.blk_first[blk] : 0u;  // wave-uniform
    e.gi = static_cast<uint64_t>(first) + (inc - e.nf);
    return e;
}

__device__ __forceinline__ uint32_t be32(uint32_t v) { return __builtin_bswap32(v); }

template <bool NT>
__global__ __launch_bounds__(64) void rx_place_kernel(const PlaceArgs a)
{
    __shared__ uint32_t pd[kPlacePd][64];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t blk = blockIdx.x;
    const uint64_t p = static_cast<uint64_t>(blk) * 64 + lane;
    const bool live = p < a.n;
    const uint32_t bmask = (1u << a.blog) - 1u;
    const uint32_t T = live ? a.len16[p] : 0u;
    const uint32_t nf = (T + bmask) >> a.blog;
    const uint32_t inc = wave_incl_scan(nf);
    const uint64_t gi = static_cast<uint64_t>(a.blk_first[blk]) + (inc - nf);
    const uint32_t stv = live ? a.status[p] : 0u;
    // accepted: the verify has found every fragment inside d_buf_idx and the pool; checked again
    // for the bytes read here, so that nothing depends on what d_status held before the call
    bool ok = live && (stv & RNS_RX_ACCEPT) && nf != 0 && gi + nf <= a.n_frags;
    uint64_t s0 = 0;
    if (ok) {
        s0 = static_cast<uint64_t>(a.buf_idx[gi]) << a.blog;
        const uint32_t len0 = min(T, bmask + 1u);
        ok = s0 <= a.pool_bytes && len0 <= a.pool_bytes - s0 && T >= 16u;
    }
    uint32_t flow = RNS_RX_NO_FLOW, seq = 0, ack = 0, ports = 0, win_pay = 0, misc = 0, place = 0;
    uint32_t skip = 0, plen = 0;
    uint64_t dst = 0;
    if (ok) {
        const uint32_t *h = reinterpret_cast<const uint32_t *>(a.pool + s0);
        const uint32_t w0 = h[0];
        const bool v6 = ((w0 >> 4) & 0xfu) == 6u;  // accepted: version 4 or 6
        const uint32_t ip_hdr = v6 ? 40u : (w0 & 0xfu) * 4u;
        // accepted: T >= 16 (IPv4) or 40 (IPv6), so the protocol and the source address are the datagram's
        const uint32_t proto = v6 ? (h[1] >> 16) & 0xffu : (h[2] >> 8) & 0xffu;
        if (proto == 6u && ip_hdr + 20u <= T) {  // L >= 20 (and so T >= 60 for IPv6: its source address is there)
            const uint32_t *t = h + (ip_hdr >> 2);
            const uint32_t t0 = t[0], t3 = t[3];
            const uint32_t tcp_hdr = ((t3 >> 4) & 0xfu) * 4u;
            if (tcp_hdr >= 20u && ip_hdr + tcp_hdr <= T) {
                place = RNS_PLACE_TCP;
                seq = be32(t[1]);
                ack = be32(t[2]);
                const uint32_t sport = ((t0 & 0xffu) << 8) | ((t0 >> 8) & 0xffu);
                const uint32_t dport = ((t0 >> 8) & 0xff00u) | (t0 >> 24);
                const uint32_t flags = (t3 >> 8) & 0xffu, window = ((t3 >> 8) & 0xff00u) | (t3 >> 24);
                skip = ip_hdr + tcp_hdr;
                plen = T - skip;
                ports = sport | (dport << 16);
                win_pay = window | (plen << 16);
                misc = flags | (ip_hdr << 8) | (tcp_hdr << 16);
                if (a.n_flows) {
                    const uint32_t key[6] = {v6 ? h[2] : h[3], v6 ? h[3] : 0u, v6 ? h[4] : 0u, v6 ? h[5] : 0u, ports,
                                             v6 ? 6u : 4u};
                    flow = flow_lookup(a, key);
                }
                if (flow != RNS_RX_NO_FLOW) {
                    place |= RNS_PLACE_FLOW;
                    if (plen != 0 && !(flags & 0x06u)) {  // data, neither SYN nor RST
                        const uint32_t d = seq - a.next_seq[flow], wl = a.win_len[flow];
                        const uint64_t wo = a.win_off[flow];
                        if (d < wl && plen <= wl - d && wo <= a.stream_bytes && wl <= a.stream_bytes - wo) {
                            place |= RNS_PLACE_DONE;
                            dst = wo + d;
                        } else {
                            place |= RNS_PLACE_OUTSIDE;
                        }
                    }
                }
            }
        }
    }
    if (live) {
        uint32_t *m = a.meta + p * 6;
        m[0] = flow;
        m[1] = seq;
        m[2] = ack;
        m[3] = ports;
        m[4] = win_pay;
        m[5] = misc | (place << 24);
    }
    // the wave's destination chunks, concatenated: at most 64 * 4097 of them
    const bool done = (place & RNS_PLACE_DONE) != 0;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(a.stream + dst) & 15u);
    const uint32_t nck = done ? (mis + plen + 15u) >> 4 : 0u;
    const uint32_t cinc = wave_incl_scan(nck);
    const uint32_t W = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cinc), 63));
    if (W == 0)
        return;
    pd[0][lane] = cinc - nck;
    pd[1][lane] = static_cast<uint32_t>(gi);
    pd[2][lane] = static_cast<uint32_t>(gi >> 32);
    pd[3][lane] = skip;
    pd[4][lane] = plen;
    pd[5][lane] = static_cast<uint32_t>(dst);
    pd[6][lane] = static_cast<uint32_t>(dst >> 32);
    wave_lds_fence();
    for (uint32_t vb = 0; vb < W; vb += 128u) {
        const PlaceChunk c0 = place_fetch<NT>(a, pd, vb + lane, W);
        const PlaceChunk c1 = place_fetch<NT>(a, pd, vb + 64u + lane, W);
        const uint4 y0 = place_second<NT>(a, c0, lane), y1 = place_second<NT>(a, c1, lane);
        place_emit(c0, y0);
        place_emit(c1, y1);
    }
}

}  // namespace rns
