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
//                           its queued payloads concatenated (pool_walk, rns_k_pool_view.hpp).
//                           Destinations are 16-byte aligned, so
//                           every chunk is one whole aligned store, a payload's last chunk with unspecified
//                           bytes after its end (its own range's slack).
// ---------------------------------------------------------------------------
// The wave's LDS table: pool_walk's rows, then a queued datagram's off16.
constexpr int kUdpPd = kPdRows + 1;

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
        // the first buffer's checks (rns_k_pool_view.hpp says why each read is safe), as this kernel's own lines
        bool ok = e.live && (stv & RNS_RX_ACCEPT) && e.nf != 0 && e.gi + e.nf <= a.rx.n_frags;
        uint32_t rec = kUdpNotDgram;
        if (ok) {
            const uint64_t s0 = static_cast<uint64_t>(a.rx.buf_idx[e.gi]) << a.rx.blog;
            const uint32_t len0 = min(e.T, 1u << a.rx.blog);
            ok = s0 <= a.rx.pool_bytes && len0 <= a.rx.pool_bytes - s0 && e.T >= 16u;
            if (ok) {
                const uint32_t *h = reinterpret_cast<const uint32_t *>(a.rx.pool + s0);
                const uint32_t w0 = h[0];
                const bool v6 = ((w0 >> 4) & 0xfu) == 6u;
                const uint32_t ip_hdr = v6 ? 40u : (w0 & 0xfu) * 4u;
                const uint32_t proto = v6 ? (h[1] >> 16) & 0xffu : (h[2] >> 8) & 0xffu;
                // the ports' dword lies in the first buffer (ip_hdr + 8 <= 68 <= B) and inside the datagram
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
            const uint32_t *h = pool_first(a.rx, e[k]);
            const IpHead ip = ip_head(h);
            const bool v6 = ip.v6;
            ip_hdr = ip.ip_hdr;
            const uint32_t sport = l4_sport(h[ip_hdr >> 2]);
            uint4 *const r = a.rec_out + 2ull * pos[k];
            r[0] = v6 ? make_uint4(h[2], h[3], h[4], h[5]) : make_uint4(h[3], 0u, 0u, 0u);
            r[1] = make_uint4(static_cast<uint32_t>(e[k].p), off[k], sport | (plen << 16), (v6 ? 6u : 4u) | (flags << 8));
        }
        // the wave's destination chunks, concatenated: at most 64 * 4096 of them
        const uint32_t nck = queued ? units : 0u;
        const uint32_t cinc = wave_incl_scan(nck);
        const uint32_t W = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cinc), 63));
        if (W != 0) {
            pool_rows(pd, lane, cinc - nck, e[k].gi, ip_hdr + 8u, plen);
            pd[kPdRows][lane] = off[k];
            wave_lds_fence();
            // the cut found the whole range inside d_data: every chunk one aligned store (the range's own slack)
            pool_walk<NT>(
                a.rx, pd, W, lane,
                [](uint32_t) { return 0u; },
                [&](uint32_t j, uint32_t c) { return a.data + 16ull * (static_cast<uint64_t>(pd[kPdRows][j]) + c); },
                [](const PlaceChunk &ck, const uint4 y) { place_emit_whole(ck, y); });
            wave_lds_fence();  // the next step writes the table again
        }
    }
}

}  // namespace rns
