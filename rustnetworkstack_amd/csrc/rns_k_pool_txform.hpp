// The pool transmit form as its builders see it (the echo responder, the UDP send build; the next ones: ICMP
// errors, pure ACKs into pool buffers, ARP and neighbour replies).  A builder is three launches on one stream: a
// classify kernel leaves a dword per item and its workgroup's sums (build_parts), scan2_parts_kernel scans them,
// and the build kernel gives every item its place (tx_alloc: free-list buffers under a cap, the totals stored by
// one lane of the grid into the zeroed d_count, no atomics), its status (tx_status), its payload chunks' addresses
// (tx_chunk_dst) and its descriptors (tx_describe).  The IP head words, the workspace's size and the local
// addresses are plain C++ that a host compiler takes (tests/cpp/test_pool_txform.cpp).
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include <cstring>

#include "rns_checksum.h"
#include "rns_k_scan.hpp"

namespace rns {

// One status byte for every builder: an item (a request, a send), then what became of it.
constexpr uint32_t kTxItem = RNS_ECHO_REQUEST, kTxBuilt = RNS_ECHO_BUILT, kTxNobuf = RNS_ECHO_NOBUF, kTxBadbuf = RNS_ECHO_BADBUF;
static_assert(RNS_UDPTX_SEND == kTxItem && RNS_UDPTX_BUILT == kTxBuilt && RNS_UDPTX_NOBUF == kTxNobuf &&
                  RNS_UDPTX_BADBUF == kTxBadbuf,
              "rns_checksum.h's echo and send bits are the same bits");

// The local addresses as they lie in memory.
struct LocalAddrs {
    uint32_t v4;
    uint32_t v6[4];
};

inline void set_local(LocalAddrs &l, const uint8_t *local_ipv4, const uint8_t *local_ipv6)
{
    std::memcpy(&l.v4, local_ipv4, 4);
    std::memcpy(l.v6, local_ipv6, 16);
}

// The workspace of a classify / scan / build sequence over n items, 8-byte aligned: two arrays of block sums
// (blocks + 1 pairs each), then a dword per item.
RNS_HD uint64_t build_work_bytes(uint64_t n) { return 16ull * (scan_blocks(n) + 1) + 4ull * n; }

// The pseudo-header's address sums.
RNS_HD uint32_t addr_sum4(uint32_t local, uint32_t peer) { return be2(local) + be2(peer); }
RNS_HD uint32_t addr_sum6(const uint32_t (&local)[4], const uint32_t (&peer)[4])
{
    return be2(local[0]) + be2(local[1]) + be2(local[2]) + be2(local[3]) + be2(peer[0]) + be2(peer[1]) + be2(peer[2]) +
           be2(peer[3]);
}

// ip_output_v4 (ip.rs:133-160): 45 00 len | id 0000 | 40 proto csum | local | peer, the header checksum filled;
// total as u16.
struct Ip4Head {
    uint32_t d[5];
};
RNS_HD Ip4Head ip4_head(uint32_t total, uint32_t id, uint32_t proto, uint32_t local, uint32_t peer)
{
    total &= 0xffffu;
    const uint32_t ttl_proto = 0x4000u + proto;
    const uint32_t ipck = fold16(0x4500u + total + id + ttl_proto + addr_sum4(local, peer)) ^ 0xffffu;
    return Ip4Head{{0x45u | (bswap16_u32(total) << 16), bswap16_u32(id), bswap16_u32(ttl_proto) | (bswap16_u32(ipck) << 16), local,
                    peer}};
}

// ip_output_v6 (ip.rs:162-177): 60 00 00 00 | len next 40 | local | peer; plen <= 0xffff.
struct Ip6Head {
    uint32_t d[10];
};
RNS_HD Ip6Head ip6_head(uint32_t plen, uint32_t next, const uint32_t (&local)[4], const uint32_t (&peer)[4])
{
    return Ip6Head{{0x60u, bswap16_u32(plen) | (next << 16) | (64u << 24), local[0], local[1], local[2], local[3], peer[0],
                    peer[1], peer[2], peer[3]}};
}

}  // namespace rns

#ifdef __HIPCC__
#include "rns_k_pool_view.hpp"

namespace rns {

// The transmit side: the pool and its free list, the descriptors a builder leaves and the counts.
struct PoolTx {
    uint8_t *tx_pool;   // 16-byte aligned
    uint64_t tx_bufs;   // whole buffers of the transmit pool
    const uint32_t *free;
    const uint32_t *ip_id_add;
    uint32_t *tx_blk_first;
    uint8_t *tx_head_len8;
    uint16_t *tx_pay_len16;
    uint32_t *tx_src;   // optional
    uint32_t *count;    // items built, buffers taken, IPv4 ids taken
    uint32_t n_free, cap, ip_id_base, blog;
};

struct BuildWork {
    uint2 *part_a;  // the workgroups' (payload buffers, items), blocks + 1
    uint2 *part_b;  // the workgroups' (IPv4 items, 0), blocks + 1
    uint32_t *rec;  // a dword per item, the classify's verdict in the family's own encoding
};

inline BuildWork carve_build_work(void *d_work, uint64_t n)
{
    BuildWork w;
    w.part_a = static_cast<uint2 *>(d_work);
    w.part_b = w.part_a + scan_blocks(n) + 1;
    w.rec = reinterpret_cast<uint32_t *>(w.part_b + scan_blocks(n) + 1);
    return w;
}

// The tail of a classify kernel (whole workgroup): the workgroup's sums of (payload buffers, items) and
// (IPv4 items, 0) for the scan between the two launches.
__device__ __forceinline__ void build_parts(const BuildWork &w, uint32_t item_bufs, uint32_t is_item, bool v4)
{
    uint2 ta, tb;
    (void)scan2_block(make_uint2(item_bufs, is_item), ta);
    (void)scan2_block(make_uint2(v4 ? 1u : 0u, 0u), tb);
    if (threadIdx.x == 0) {
        w.part_a[blockIdx.x] = ta;
        w.part_b[blockIdx.x] = tb;
    }
}

// The IPv4 identification of the item with v4_before IPv4 items built before it.
__device__ __forceinline__ uint32_t ip_id(uint32_t ip_id_base, const uint32_t *ip_id_add, uint32_t v4_before)
{
    return (ip_id_base + (ip_id_add ? *ip_id_add : 0u) + v4_before) & 0xffffu;
}

// An item's place in the transmit form: its rank r among the items, its first buffer's place fi in the free
// list (the head buffer; the payload's nfr - 1 follow), the IPv4 items before it, whether it is built (within
// the cap and the free list) and, if so, whether one of its buffers lies outside the pool.
struct TxSlot {
    uint32_t r, fi, nfr, v4_before;
    bool built, bad;
};

// The allocation (whole workgroup, every thread of the grid once): scans the workgroup again, adds the scanned
// block sums, applies the cap and the free list's length — both counts are monotone, so the built items are a
// prefix of the items — and stores the totals.  early(built) runs once an item knows whether it is built, before
// its buffers are looked at: a builder issues the loads it needs of a built item there, ahead of the free list's.
template <class Early>
__device__ __forceinline__ TxSlot tx_alloc(const PoolTx &tx, const BuildWork &w, bool is_item, uint32_t pbufs, bool v4, Early early)
{
    uint2 ta, tb;
    const uint2 xa = scan2_block(make_uint2(pbufs, is_item ? 1u : 0u), ta);
    const uint2 xb = scan2_block(make_uint2(v4 ? 1u : 0u, 0u), tb);
    const uint2 ca = w.part_a[blockIdx.x], cb = w.part_b[blockIdx.x];
    // exclusive counts before this item: items, their buffers (64 bits), IPv4 items
    const uint32_t r = ca.y + xa.y, v4_before = cb.x + xb.x;
    const uint64_t f0 = static_cast<uint64_t>(ca.x + xa.x) + r;
    const uint32_t nfr = 1u + pbufs;
    const bool built = is_item && r < tx.cap && f0 + nfr <= tx.n_free;
    const uint32_t fi = static_cast<uint32_t>(f0);  // built: f0 < n_free
    early(built);
    bool bad = false;
    if (built) {
        for (uint32_t k = 0; k < nfr; ++k)
            bad = bad || tx.free[fi + k] >= tx.tx_bufs;
    }
    // the totals, stored by one lane of the grid: the first item that is not built holds them as its exclusive
    // counts (its predecessor was built: r - 1 < cap and f0 <= n_free), and when every item is built the last
    // one holds them as its inclusive counts.  (No item built: the zeroed d_count stands.)
    if (is_item && (built ? r + 1u == w.part_a[gridDim.x].y : r != 0 && r - 1u < tx.cap && f0 <= tx.n_free)) {
        tx.count[0] = r + (built ? 1u : 0u);
        tx.count[1] = fi + (built ? nfr : 0u);
        tx.count[2] = v4_before + (built && v4 ? 1u : 0u);
    }
    return TxSlot{r, fi, nfr, v4_before, built, bad};
}

__device__ __forceinline__ uint8_t tx_status(const TxSlot &s, bool is_item)
{
    return static_cast<uint8_t>(!is_item ? 0u : !s.built ? kTxItem | kTxNobuf : s.bad ? kTxItem | kTxBadbuf : kTxItem | kTxBuilt);
}

// Chunk c (16 bytes) of the payload whose first buffer is d_free[first_free]: it lies in buffer
// c >> (blog - 4).  (The item's buffers were found inside the transmit pool before its chunks were counted.)
__device__ __forceinline__ uint8_t *tx_chunk_dst(const PoolTx &tx, uint32_t first_free, uint32_t c)
{
    const uint32_t bi = tx.free[first_free + (c >> (tx.blog - 4u))];
    return tx.tx_pool + (static_cast<uint64_t>(bi) << tx.blog) + ((16u * c) & ((1u << tx.blog) - 1u));
}

// A built item's descriptors, stored by its owner lane.  Returns the end of its head buffer, where the head's
// last byte goes; null for an item with a bad buffer, whose head length is 0.
__device__ __forceinline__ uint8_t *tx_describe(const PoolTx &tx, const TxSlot &s, uint32_t head_len, uint32_t pay_len, uint64_t src)
{
    tx.tx_head_len8[s.r] = static_cast<uint8_t>(s.bad ? 0u : head_len);
    tx.tx_pay_len16[s.r] = static_cast<uint16_t>(pay_len);
    if (tx.tx_src)
        tx.tx_src[s.r] = static_cast<uint32_t>(src);
    if ((s.r & 63u) == 0)
        tx.tx_blk_first[s.r >> 6] = s.fi;
    if (s.bad)
        return nullptr;
    return tx.tx_pool + (static_cast<uint64_t>(tx.free[s.fi]) << tx.blog) + (1u << tx.blog);
}

}  // namespace rns
#endif  // __HIPCC__
