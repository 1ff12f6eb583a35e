// UDP receive demux over pool buffers (rns_rx_udp_demux_pool_dev): udp_input's socket queues, built on the
// device from a verified receive batch.
// (The kernels of k_udp.hip alone: three of them are no templates.  Their arguments are in rns_k_args.hpp.)
#pragma once

#include "rns_k_args.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// udp_input (udp.rs:126-148) reads the ports, looks the destination port up in PORT_MAP and pushes
// (source address, source port, payload) onto that socket's receive_queue.  A datagram's place in its
// queue is its rank among the earlier datagrams of the same socket: a stable grouping of the batch by
// socket.  Here the pool verify runs as it is, then five more launches on the same stream; grid-wide
// ordering comes from the launch boundaries only, and no atomic's order reaches an output (the one
// atomic is an integer add into a workgroup's LDS histogram):
//   1. udp_classify_kernel  a lane per datagram, a wave per 64-datagram block (the unit of d_blk_first),
//                           a workgroup per tile of kUdpTile datagrams: reads the status and the first
//                           buffer's header dwords, looks the destination port up, leaves one dword per
//                           datagram in the workspace (socket, payload bytes) and the tile's per-socket
//                           (entries, 16-byte units) in the counts matrix, socket-major: element
//                           s * n_tiles + t, zeros included.
//   2. scan2_reduce_kernel, scan2_parts_kernel (rns_k_scan.hpp) and udp_prefix_kernel over the matrix as
//                           one sequence of n_socks * n_tiles pairs: the exclusive prefix at (s, t) is the
//                           record position and the unit offset of tile t's first entry for socket s, the
//                           prefix at (s, 0) is d_q_first[s], the total is d_count.
//   3. udp_scatter_kernel   per tile: every datagram's rank and unit prefix among its socket's datagrams
//                           of its own wave and step (a loop over the wave's distinct sockets: ballot, a
//                           masked prefix sum), then the waves in batch order add the socket's running
//                           (entries, units) from LDS — it starts as the matrix prefix — and leave it
//                           advanced for the next step and wave.  The cut, the record as two 16-byte
//                           stores, d_udp, d_pos; then each wave walks the destination 16-byte chunks of all
//                           its queued payloads concatenated, the placement's walk (place_owner /
//                           place_load / place_second / place_join).  Destinations are 16-byte aligned, so
//                           every chunk is one whole aligned store, a payload's last chunk with unspecified
//                           bytes after its end (its own range's slack).
// ---------------------------------------------------------------------------
constexpr int kUdpPd = 6;
// Per queued datagram in the wave's LDS table: [0] the wave's destination chunks before it, [1] [2] its
// first fragment's place in d_buf_idx, [3] ip_hdr + 8, [4] payload bytes, [5] off16.

// The 64-datagram block of wave wv's step k in tile `tile`: a wave's blocks are consecutive, so batch order
// is the waves in order, each one's steps in order.
__device__ __forceinline__ uint32_t udp_block(uint32_t tile, uint32_t wv, uint32_t k)
{
    return (tile * kUdpWaves + wv) * kUdpSteps + k;
}

__global__ __launch_bounds__(kScanBlock) void udp_classify_kernel(const UdpArgs a)
{
    __shared__ unsigned long long hist[RNS_UDP_MAX_SOCKS];  // entries | units << 32
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint32_t s = threadIdx.x; s < a.n_socks; s += kScanBlock)
        hist[s] = 0ull;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kUdpSteps; ++k) {
        const PoolLane e = pool_lane(a.rx, udp_block(blockIdx.x, wv, k), lane);
        const uint32_t stv = e.live ? a.rx.status[e.p] : 0u;
        // accepted: the verify has found every fragment inside d_buf_idx and the pool; checked again for the
        // bytes read here and in the scatter, so that nothing depends on what d_status held before the call
        bool ok = e.live && (stv & RNS_RX_ACCEPT) && e.nf != 0 && e.gi + e.nf <= a.rx.n_frags;
        uint32_t rec = kUdpNotDgram;
        if (ok) {
            const uint64_t s0 = static_cast<uint64_t>(a.rx.buf_idx[e.gi]) << a.rx.blog;
            const uint32_t len0 = min(e.T, 1u << a.rx.blog);
            ok = s0 <= a.rx.pool_bytes && len0 <= a.rx.pool_bytes - s0 && e.T >= 16u;
            if (ok) {
                const uint32_t *h = reinterpret_cast<const uint32_t *>(a.rx.pool + s0);
                const uint32_t w0 = h[0];
                const bool v6 = ((w0 >> 4) & 0xfu) == 6u;  // accepted: version 4 or 6
                const uint32_t ip_hdr = v6 ? 40u : (w0 & 0xfu) * 4u;
                // accepted: T >= 16 (IPv4) or 40 (IPv6), so the protocol is the datagram's; the ports' dword lies
                // in the first buffer (ip_hdr + 8 <= 68 <= B) and inside the datagram
                const uint32_t proto = v6 ? (h[1] >> 16) & 0xffu : (h[2] >> 8) & 0xffu;
                if (proto == 17u && ip_hdr + 8u <= e.T) {
                    const uint32_t t0 = h[ip_hdr >> 2];
                    const uint32_t dport = ((t0 >> 8) & 0xff00u) | (t0 >> 24);
                    const uint32_t s = a.n_socks ? a.port_tbl[dport] : kUdpNoSock;
                    rec = (s < a.n_socks ? s : kUdpNoSock) | ((e.T - ip_hdr - 8u) << 16);
                }
            }
        }
        if (e.live)
            a.rec[e.p] = rec;
        const uint32_t s = rec & 0xffffu;
        if (s < a.n_socks)  // an integer sum: the same whatever the order
            atomicAdd(&hist[s], 1ull | (static_cast<unsigned long long>(((rec >> 16) + 15u) >> 4) << 32));
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < a.n_socks; s += kScanBlock) {
        const unsigned long long v = hist[s];
        a.mat[static_cast<uint64_t>(s) * a.n_tiles + blockIdx.x] =
            make_uint2(static_cast<uint32_t>(v), static_cast<uint32_t>(v >> 32));
    }
}

// the scan's value: the matrix as one sequence
struct UdpMatValue {
    static __device__ __forceinline__ uint2 value(const UdpArgs &a, uint64_t i) { return a.mat[i]; }
};

// The matrix to its exclusive prefix sums, in place (part[] holds the blocks' prefixes), and d_q_first.
__global__ __launch_bounds__(kScanBlock) void udp_prefix_kernel(const UdpArgs a, uint64_t m)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    const uint2 v = i < m ? a.mat[i] : make_uint2(0u, 0u);
    uint2 total;
    const uint2 ex = scan2_block(v, total);
    const uint2 before = a.part[blockIdx.x];
    if (i < m) {
        a.mat[i] = make_uint2(before.x + ex.x, before.y + ex.y);
        if (i % a.n_tiles == 0)
            a.q_first[i / a.n_tiles] = before.x + ex.x;
    }
    if (i == 0)
        a.q_first[a.n_socks] = a.part[gridDim.x].x;
}

// A datagram's rank and unit prefix among the datagrams of the same socket in its wave, and whether it is
// the last of them.  (Called by the whole wave; the loop runs once per distinct socket.)
struct UdpRank {
    uint32_t rank, ubefore;
    bool last;
};

__device__ __forceinline__ UdpRank udp_wave_rank(bool has, uint32_t sock, uint32_t units, uint32_t lane)
{
    UdpRank r{0u, 0u, false};
    uint64_t todo = __ballot(has);
    while (todo) {
        const int first = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
        const uint32_t s0 = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(sock), first));
        const bool mine = has && sock == s0;
        const uint64_t m = __ballot(mine);
        const uint32_t inc = wave_incl_scan(mine ? units : 0u);  // <= 64 * 4096
        if (mine) {
            r.rank = static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
            r.ubefore = inc - units;
            r.last = (m >> lane) == 1ull;
        }
        todo &= ~m;
    }
    return r;
}

// Chunk v of the wave's concatenated destination chunks, its first load issued: place_fetch with the
// destination at the payload's 16-byte-aligned place in d_data.
template <bool NT>
__device__ __forceinline__ PlaceChunk udp_fetch(const UdpArgs &a, const uint32_t (&pd)[kUdpPd][64], uint32_t v, uint32_t W)
{
    PlaceChunk ck{};
    ck.j = ~0u;
    if (v >= W)
        return ck;
    const uint32_t j = place_owner(pd, v);
    const uint32_t c = v - pd[0][j], skip = pd[3][j], plen = pd[4][j];
    const uint64_t gi = (static_cast<uint64_t>(pd[2][j]) << 32) | pd[1][j];
    const uint32_t o0 = skip + 16u * c;  // < skip + plen = T <= 65535
    const uint32_t s = o0 & ~15u;
    ck.sh = o0 & 15u;
    ck.x = place_load<NT>(a.rx, gi, s);
    ck.s2 = (ck.sh && s + 16u < skip + plen) ? s + 16u : 0u;
    ck.gi = gi;
    ck.j = j;
    ck.dc = a.data + 16ull * (static_cast<uint64_t>(pd[5][j]) + c);  // the cut found the whole range inside d_data
    ck.lo = 0u;
    ck.hi = min(16u, plen - 16u * c);  // >= 1: c is below the payload's chunk count
    return ck;
}

// The chunk as one aligned store: whole also where the payload ends inside it (the slack of its own range).
__device__ __forceinline__ void udp_emit(const PlaceChunk &ck, const uint4 y)
{
    if (ck.hi == 0)
        return;
    uint32_t o[4];
    place_join(ck, y, o);
    *reinterpret_cast<uint4 *>(ck.dc) = make_uint4(o[0], o[1], o[2], o[3]);
}

template <bool NT>
__global__ __launch_bounds__(kScanBlock) void udp_scatter_kernel(const UdpArgs a)
{
    __shared__ uint2 base[RNS_UDP_MAX_SOCKS];  // per socket: the next record position and unit offset
    __shared__ uint32_t pds[kUdpWaves][kUdpPd][64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t(&pd)[kUdpPd][64] = pds[wv];
    for (uint32_t s = threadIdx.x; s < a.n_socks; s += kScanBlock)
        base[s] = a.mat[static_cast<uint64_t>(s) * a.n_tiles + blockIdx.x];
    PoolLane e[kUdpSteps];
    uint32_t rec[kUdpSteps], pos[kUdpSteps], off[kUdpSteps];
    UdpRank rk[kUdpSteps];
#pragma unroll
    for (uint32_t k = 0; k < kUdpSteps; ++k) {
        e[k] = pool_lane(a.rx, udp_block(blockIdx.x, wv, k), lane);
        rec[k] = e[k].live ? a.rec[e[k].p] : kUdpNotDgram;
        const bool has = (rec[k] & 0xffffu) < a.n_socks;
        rk[k] = udp_wave_rank(has, rec[k] & 0xffffu, ((rec[k] >> 16) + 15u) >> 4, lane);
        pos[k] = off[k] = 0u;
    }
    __syncthreads();
    // the waves in batch order, each one's steps in order: the socket's running counts, then advanced by the
    // last of the socket's datagrams in the step (its inclusive counts are the step's totals)
    for (uint32_t w = 0; w < kUdpWaves; ++w) {
        if (wv == w) {
#pragma unroll
            for (uint32_t k = 0; k < kUdpSteps; ++k) {
                const uint32_t s = rec[k] & 0xffffu;
                if (s < a.n_socks) {
                    const uint2 b = base[s];
                    pos[k] = b.x + rk[k].rank;
                    off[k] = b.y + rk[k].ubefore;
                    if (rk[k].last)
                        base[s] = make_uint2(pos[k] + 1u, off[k] + (((rec[k] >> 16) + 15u) >> 4));
                }
                wave_lds_fence();
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (uint32_t k = 0; k < kUdpSteps; ++k) {
        const uint32_t s = rec[k] & 0xffffu, plen = rec[k] >> 16, units = (plen + 15u) >> 4;
        const bool has = s < a.n_socks;
        const bool queued = has && pos[k] < a.rec_cap && 16ull * (static_cast<uint64_t>(off[k]) + units) <= a.data_bytes;
        const uint32_t flags = s == kUdpNotDgram ? 0u
                               : !has            ? RNS_UDP_DGRAM
                                                 : RNS_UDP_DGRAM | RNS_UDP_SOCK | (queued ? RNS_UDP_QUEUED : RNS_UDP_NOROOM);
        if (e[k].live) {
            a.udp[e[k].p] = static_cast<uint8_t>(flags);
            if (a.pos)
                a.pos[e[k].p] = queued ? pos[k] : 0xffffffffu;
        }
        uint32_t ip_hdr = 0;
        if (queued) {
            // the record: the classify found these header dwords inside the first buffer and the pool
            const uint32_t *h =
                reinterpret_cast<const uint32_t *>(a.rx.pool + (static_cast<uint64_t>(a.rx.buf_idx[e[k].gi]) << a.rx.blog));
            const uint32_t w0 = h[0];
            const bool v6 = ((w0 >> 4) & 0xfu) == 6u;
            ip_hdr = v6 ? 40u : (w0 & 0xfu) * 4u;
            const uint32_t t0 = h[ip_hdr >> 2];
            const uint32_t sport = ((t0 & 0xffu) << 8) | ((t0 >> 8) & 0xffu);
            uint4 *const r = a.rec_out + 2ull * pos[k];
            r[0] = v6 ? make_uint4(h[2], h[3], h[4], h[5]) : make_uint4(h[3], 0u, 0u, 0u);
            r[1] = make_uint4(static_cast<uint32_t>(e[k].p), off[k], sport | (plen << 16), (v6 ? 6u : 4u) | (flags << 8));
        }
        // the wave's destination chunks, concatenated: at most 64 * 4096 of them
        const uint32_t nck = queued ? units : 0u;
        const uint32_t cinc = wave_incl_scan(nck);
        const uint32_t W = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cinc), 63));
        if (W != 0) {
            pd[0][lane] = cinc - nck;
            pd[1][lane] = static_cast<uint32_t>(e[k].gi);
            pd[2][lane] = static_cast<uint32_t>(e[k].gi >> 32);
            pd[3][lane] = ip_hdr + 8u;
            pd[4][lane] = plen;
            pd[5][lane] = off[k];
            wave_lds_fence();
            for (uint32_t vb = 0; vb < W; vb += 128u) {
                const PlaceChunk c0 = udp_fetch<NT>(a, pd, vb + lane, W);
                const PlaceChunk c1 = udp_fetch<NT>(a, pd, vb + 64u + lane, W);
                const uint4 y0 = place_second<NT>(a.rx, c0, lane), y1 = place_second<NT>(a.rx, c1, lane);
                udp_emit(c0, y0);
                udp_emit(c1, y1);
            }
            wave_lds_fence();  // the next step writes the table again
        }
    }
}

}  // namespace rns
