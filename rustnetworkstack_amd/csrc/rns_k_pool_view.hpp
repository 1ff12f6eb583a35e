// A verified pool receive batch as its consumers see it (the TCP placement, the echo responder, the UDP
// demux): the view struct, a lane's datagram, the first buffer's header arithmetic (plain C++
// that a host compiler takes: tests/cpp/test_pool_view.cpp) and the walk that copies a wave's payloads.
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_tcp_head.hpp"

namespace rns {

// What the first dwords of an IP header say, for a datagram the verify accepted (version 4 or 6,
// T >= 16 for IPv4 and 40 for IPv6, so h[0..2] are the datagram's).
struct IpHead {
    bool v6;
    uint32_t ip_hdr, proto;
};

RNS_HD IpHead ip_head(const uint32_t *h)
{
    const uint32_t w0 = h[0];
    IpHead d;
    d.v6 = ((w0 >> 4) & 0xfu) == 6u;
    d.ip_hdr = d.v6 ? 40u : (w0 & 0xfu) * 4u;
    d.proto = d.v6 ? (h[1] >> 16) & 0xffu : (h[2] >> 8) & 0xffu;
    return d;
}

// The ports of a TCP or UDP header's first dword as it lies in memory.
RNS_HD uint32_t l4_sport(uint32_t t0) { return ((t0 & 0xffu) << 8) | ((t0 >> 8) & 0xffu); }
RNS_HD uint32_t l4_dport(uint32_t t0) { return ((t0 >> 8) & 0xff00u) | (t0 >> 24); }

}  // namespace rns

#ifdef __HIPCC__
#include "rns_k_pool_rx.hpp"

namespace rns {

// The pool receive form, with the verify's verdicts.
struct PoolRx {
    const uint8_t *pool;  // 16-byte aligned
    uint64_t pool_bytes;
    const uint32_t *buf_idx;
    const uint32_t *blk_first;
    const uint16_t *len16;
    const uint8_t *status;
    uint32_t n, n_frags, blog;
};

// A datagram's place in the pool form, as the verify computes it (whole wave): a wave owns one 64-datagram block,
// the unit of d_blk_first; a lane's first fragment is d_blk_first[block] + the DPP prefix sum of the fragment counts.
struct PoolLane {
    uint64_t p, gi;
    uint32_t T, nf;
    bool live;
};

__device__ __forceinline__ PoolLane pool_lane(const PoolRx &rx, uint32_t blk, uint32_t lane)
{
    PoolLane e;
    e.p = static_cast<uint64_t>(blk) * 64 + lane;
    e.live = e.p < rx.n;
    const uint32_t bmask = (1u << rx.blog) - 1u;
    e.T = e.live ? rx.len16[e.p] : 0u;
    e.nf = (e.T + bmask) >> rx.blog;
    const uint32_t inc = wave_incl_scan(e.nf);
    const uint32_t first = static_cast<uint64_t>(blk) * 64 < rx.n ? rx.blk_first[blk] : 0u;  // wave-uniform
    e.gi = static_cast<uint64_t>(first) + (inc - e.nf);
    return e;
}

// The first buffer's checks, which the placement and the two classify kernels each make in lines of their own
// (DESIGN.md "One view of a verified pool batch") before they read header dwords.  Accepted means that the verify
// has found every fragment inside d_buf_idx and the pool; both are checked again (gi + nf <= n_frags, the first
// buffer's bytes inside the pool), so that nothing depends on what d_status held before the call.  T >= 16 makes
// h[0..3] the datagram's; accepted, it has T >= 16 (IPv4) or 40 (IPv6), so the protocol and the source address are
// its own, and the L4 header's first 20 / 8 / 4 bytes lie in the first buffer once B holds them (each consumer's
// minimum buf_log2) and inside the datagram once ip_hdr + that many <= T, which the consumer checks.
// pool_first: the first buffer as dwords, for a datagram that passed those checks in an earlier kernel of the call.
__device__ __forceinline__ const uint32_t *pool_first(const PoolRx &rx, const PoolLane &e)
{
    return reinterpret_cast<const uint32_t *>(rx.pool + (static_cast<uint64_t>(rx.buf_idx[e.gi]) << rx.blog));
}

// The copy, the whole wave on its datagrams together.  Every destination range is cut into its
// 16-byte-aligned chunks and the wave walks the chunks of all its datagrams concatenated (the prefix sum
// of the chunk counts in LDS, a six-step search per chunk), 128 at a time with both halves' loads in
// flight, so short payloads fill the lanes as well as long ones.  A destination chunk draws on the two
// aligned source chunks around the same payload bytes (each inside one buffer, B a multiple of 16: one
// index load per chunk), joined at the byte shift (source offset - destination address) & 15, which is the
// same for every chunk of a datagram; the second of the two is the next destination chunk's first, so a
// lane takes it from the next lane where that lane holds the same datagram and loads it only at a
// datagram's or the wave's edge.  A source chunk that is not whole inside the pool (the tail of a pool
// whose size is no multiple of 16) is read byte by byte.

// The wave's LDS table, a row of 64 per field, what the walk needs of each datagram it copies: the wave's chunks
// before it, its first fragment's place in d_buf_idx (two rows), the header bytes before its payload, the
// payload's bytes.  A consumer's own rows (where the payload goes) follow from kPdRows on.
constexpr int kPdBefore = 0, kPdGiLo = 1, kPdGiHi = 2, kPdSkip = 3, kPdLen = 4, kPdRows = 5;

template <int ROWS>
__device__ __forceinline__ void pool_rows(uint32_t (&pd)[ROWS][64], uint32_t lane, uint32_t before, uint64_t gi, uint32_t skip,
                                          uint32_t plen)
{
    pd[kPdBefore][lane] = before;
    pd[kPdGiLo][lane] = static_cast<uint32_t>(gi);
    pd[kPdGiHi][lane] = static_cast<uint32_t>(gi >> 32);
    pd[kPdSkip][lane] = skip;
    pd[kPdLen][lane] = plen;
}

// The aligned 16-byte chunk at byte s of the datagram whose fragments start at d_buf_idx[gi]
// (s below the datagram's length, so the fragment exists); bytes outside the pool read as zero.
template <bool NT>
__device__ __forceinline__ uint4 place_load(const PoolRx &a, uint64_t gi, uint32_t s)
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

// One destination chunk: the first of the two source chunks around its bytes, and where they go.
struct PlaceChunk {
    uint4 x;
    uint64_t gi;        // its datagram's first fragment
    uint8_t *dc;        // the chunk's 16-byte-aligned address
    uint32_t lo, hi;    // its payload bytes are [lo, hi); hi == 0: no chunk
    uint32_t sh;        // (source offset - destination address) & 15
    uint32_t s2;        // the second source chunk's offset in the datagram, 0: not needed
    uint32_t j;         // its datagram's lane, ~0: no chunk
    uint32_t c;         // its index among its datagram's chunks
};

// The datagram that owns chunk v of the wave's concatenated destination chunks: the last one whose chunks
// start at or before v.
template <int ROWS>
__device__ __forceinline__ uint32_t place_owner(const uint32_t (&pd)[ROWS][64], uint32_t v)
{
    uint32_t j = 0;
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1)
        j += pd[kPdBefore][j + step] <= v ? step : 0u;
    return j;
}

// Chunk v of the wave's concatenated destination chunks, its first load issued.  mis(j): the first byte & 15 of lane
// j's destination range; dst(j, c): its chunk c's aligned address (asked for after the load: it may load itself).
template <bool NT, int ROWS, class Mis, class Dst>
__device__ __forceinline__ PlaceChunk pool_chunk(const PoolRx &rx, const uint32_t (&pd)[ROWS][64], uint32_t v, uint32_t W,
                                                 Mis mis, Dst dst)
{
    PlaceChunk ck{};
    ck.j = ~0u;
    if (v >= W)
        return ck;
    const uint32_t j = place_owner(pd, v);
    const uint32_t c = v - pd[kPdBefore][j], skip = pd[kPdSkip][j], plen = pd[kPdLen][j];
    const uint64_t gi = (static_cast<uint64_t>(pd[kPdGiHi][j]) << 32) | pd[kPdGiLo][j];
    const uint32_t m = mis(j);
    const uint32_t o0 = skip - m + 16u * c;  // skip >= 24 > m (an IP header and 4 bytes or more); < skip + plen <= 65535
    const uint32_t s = o0 & ~15u;
    ck.sh = o0 & 15u;
    ck.x = place_load<NT>(rx, gi, s);
    ck.s2 = (ck.sh && s + 16u < skip + plen) ? s + 16u : 0u;
    ck.gi = gi;
    ck.j = j;
    ck.c = c;
    ck.dc = dst(j, c);
    ck.lo = c == 0 ? m : 0u;
    ck.hi = min(16u, m + plen - 16u * c);  // >= 1: c is below the datagram's chunk count
    return ck;
}

// The second source chunk.  The next lane's chunk, when it is the same datagram's, is the next
// destination chunk, whose first source chunk is this one's second: taken from that lane instead of
// memory.  (Called by the whole wave.)
template <bool NT>
__device__ __forceinline__ uint4 place_second(const PoolRx &a, const PlaceChunk &ck, uint32_t lane)
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

// Whole chunks go out as one aligned 16-byte store; the first and last chunk of a range, where not whole,
// as byte stores, so that two ranges that meet inside a 16-byte granule never write each other's bytes.
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

// place_emit for a range that starts 16-byte aligned and owns the slack after its end: every chunk whole.
__device__ __forceinline__ void place_emit_whole(PlaceChunk ck, const uint4 y)
{
    ck.hi = ck.hi ? 16u : 0u;
    place_emit(ck, y);
}

// A chunk's word sum added to its datagram's in the LDS row `row`, for the builders that checksum what they
// copy (the echo responder, the UDP send build): lane by lane the wave holds 64 consecutive chunks of its
// concatenated datagrams, this lane chunk c of datagram j (has: it holds one).  A datagram's chunks are
// consecutive lanes, so its sum over this step is a range of the wave's prefix sum (DPP, no LDS round trip),
// as the rows kernels take a packet's: the datagram's last lane of the step subtracts the prefix before its
// first lane — lane - min(c, lane) — and adds the range.  (Called by the whole wave.)
__device__ __forceinline__ void wave_dgram_sum(uint32_t sum, uint32_t j, uint32_t c, bool has, uint32_t lane, uint32_t (&row)[64])
{
    const uint32_t S = wave_incl_scan(sum);  // <= 64 * 8 * 0xffff
    const uint32_t a = lane - min(c, lane);
    const uint32_t before = static_cast<uint32_t>(__shfl(static_cast<int>(S), static_cast<int>(max(a, 1u)) - 1, 64));
    const uint32_t jn = static_cast<uint32_t>(__shfl_down(static_cast<int>(j), 1, 64));
    if (has && (lane == 63u || jn != j))
        row[j] += S - (a ? before : 0u);  // one lane per datagram; a payload's sum stays below 4096 * 8 * 0xffff < 2^32
    wave_lds_fence();
}

// The walk over the wave's W concatenated destination chunks (W wave-uniform, the table written and
// fenced): mis and dst say where a chunk goes (pool_chunk), emit(chunk, second source chunk) stores it.
template <bool NT, int ROWS, class Mis, class Dst, class Emit>
__device__ __forceinline__ void pool_walk(const PoolRx &rx, const uint32_t (&pd)[ROWS][64], uint32_t W, uint32_t lane, Mis mis,
                                          Dst dst, Emit emit)
{
    for (uint32_t vb = 0; vb < W; vb += 128u) {
        const PlaceChunk c0 = pool_chunk<NT>(rx, pd, vb + lane, W, mis, dst);
        const PlaceChunk c1 = pool_chunk<NT>(rx, pd, vb + 64u + lane, W, mis, dst);
        const uint4 y0 = place_second<NT>(rx, c0, lane), y1 = place_second<NT>(rx, c1, lane);
        emit(c0, y0);
        emit(c1, y1);
    }
}

}  // namespace rns
#endif  // __HIPCC__
