// TCP receive placement over pool buffers (rns_rx_tcp_place_pool_dev): tcp_input's decode, the
// PORT_MAP lookup and tcp_read's copy, for datagrams the pool receive verify has judged.
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_pool_view.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// The entry point runs rx_pool_kernel as it is (d_status / d_l4_sum are rns_rx_verify_pool_dev's by
// construction, and its instantiations keep their instructions) and then this kernel on the same
// stream, which reads the statuses back.  A wave owns one 64-datagram block (pool_lane).
//
// Decode and lookup, one datagram per lane.  An accepted datagram's IP header and the fixed 20
// TCP bytes (at most 60 + 20) lie in its first buffer (B >= 128), 4-byte aligned, and inside the
// datagram once L >= 20: the lane reads them as dwords where they lie — its first dword
// for the header length, the TCP header's five, the source address — a few lines the verify has just
// pulled through L2.  The flow table is an open-addressed hash of 32-byte slots built by
// rns_rx_flow_table_build (k_place.hip); a probe ends at an empty slot or after `slots` steps,
// and a stored flow index >= n_flows never matches, so any table bytes are safe to read.
//
// Placement, the whole wave on its placed datagrams together: pool_walk (rns_k_pool_view.hpp) with the
// destination anywhere in d_stream, so a payload's first and last chunk, where not whole, go out as byte
// stores (place_emit).
// ---------------------------------------------------------------------------
constexpr uint32_t kPlaceMinLog2 = 7;  // 60 + 60 header bytes lie inside the first buffer
static_assert((1u << kPlaceMinLog2) >= 60u + 60u, "IP and TCP headers lie inside the first buffer");

constexpr uint32_t kFlowSlotBytes = 32, kFlowSlotWords = 8, kFlowMinSlots = 64;

// (The view's fields lie flat and rx() builds the PoolRx: a PoolRx member split the arguments' scalar loads anew.)
struct PlaceArgs {
    const uint8_t *pool;
    uint64_t pool_bytes;
    const uint32_t *buf_idx;
    const uint32_t *blk_first;
    const uint16_t *len16;
    const uint8_t *status;
    const uint32_t *tbl;  // the flow table's slots
    const uint32_t *next_seq;
    const uint64_t *win_off;
    const uint32_t *win_len;
    uint8_t *stream;
    uint64_t stream_bytes;
    uint32_t *meta;  // 6 dwords per datagram
    uint32_t n, n_frags, n_flows, slots, blog;
    __host__ __device__ PoolRx rx() const { return PoolRx{pool, pool_bytes, buf_idx, blk_first, len16, status, n, n_frags, blog}; }
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

__device__ __forceinline__ uint32_t be32(uint32_t v) { return __builtin_bswap32(v); }

// The wave's LDS table: pool_walk's rows, then a placed datagram's place in d_stream.
constexpr int kPlacePd = kPdRows + 2;

template <bool NT>
__global__ __launch_bounds__(64) void rx_place_kernel(const PlaceArgs a)
{
    __shared__ uint32_t pd[kPlacePd][64];
    const uint32_t lane = threadIdx.x & 63;
    const PoolRx rx = a.rx();
    // pool_lane's lines and the first buffer's checks as this kernel's own (rns_k_pool_view.hpp says why each read
    // is safe: accepted, gi + nf <= n_frags, first buffer inside the pool, T >= 16)
    const uint32_t blk = blockIdx.x;
    const uint64_t p = static_cast<uint64_t>(blk) * 64 + lane;
    const bool live = p < rx.n;
    const uint32_t bmask = (1u << rx.blog) - 1u;
    const uint32_t T = live ? rx.len16[p] : 0u;
    const uint32_t nf = (T + bmask) >> rx.blog;
    const uint32_t inc = wave_incl_scan(nf);
    const uint64_t gi = static_cast<uint64_t>(rx.blk_first[blk]) + (inc - nf);
    const uint32_t stv = live ? rx.status[p] : 0u;
    bool ok = live && (stv & RNS_RX_ACCEPT) && nf != 0 && gi + nf <= rx.n_frags;
    uint64_t s0 = 0;
    if (ok) {
        s0 = static_cast<uint64_t>(rx.buf_idx[gi]) << rx.blog;
        const uint32_t len0 = min(T, bmask + 1u);
        ok = s0 <= rx.pool_bytes && len0 <= rx.pool_bytes - s0 && T >= 16u;
    }
    uint32_t flow = RNS_RX_NO_FLOW, seq = 0, ack = 0, ports = 0, win_pay = 0, misc = 0, place = 0;
    uint32_t skip = 0, plen = 0;
    uint64_t dst = 0;
    if (ok) {
        const uint32_t *h = reinterpret_cast<const uint32_t *>(rx.pool + s0);
        const IpHead ip = ip_head(h);
        const bool v6 = ip.v6;
        const uint32_t ip_hdr = ip.ip_hdr;
        if (ip.proto == 6u && ip_hdr + 20u <= T) {  // L >= 20 (and so T >= 60 for IPv6: its source address is there)
            const uint32_t *t = h + (ip_hdr >> 2);
            const uint32_t t0 = t[0], t3 = t[3];
            const uint32_t tcp_hdr = ((t3 >> 4) & 0xfu) * 4u;
            if (tcp_hdr >= 20u && ip_hdr + tcp_hdr <= T) {
                place = RNS_PLACE_TCP;
                seq = be32(t[1]);
                ack = be32(t[2]);
                const uint32_t flags = (t3 >> 8) & 0xffu, window = ((t3 >> 8) & 0xff00u) | (t3 >> 24);
                skip = ip_hdr + tcp_hdr;
                plen = T - skip;
                ports = l4_sport(t0) | (l4_dport(t0) << 16);
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
    pool_rows(pd, lane, cinc - nck, gi, skip, plen);
    pd[kPdRows][lane] = static_cast<uint32_t>(dst);
    pd[kPdRows + 1][lane] = static_cast<uint32_t>(dst >> 32);
    wave_lds_fence();
    // where lane j's payload goes
    const auto at = [&](uint32_t j) { return a.stream + ((static_cast<uint64_t>(pd[kPdRows + 1][j]) << 32) | pd[kPdRows][j]); };
    pool_walk<NT>(
        rx, pd, W, lane,
        [&](uint32_t j) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(at(j)) & 15u); },
        [&](uint32_t j, uint32_t c) { return at(j) - (reinterpret_cast<uintptr_t>(at(j)) & 15u) + 16ull * c; },
        [](const PlaceChunk &ck, const uint4 y) { place_emit(ck, y); });
}

}  // namespace rns
