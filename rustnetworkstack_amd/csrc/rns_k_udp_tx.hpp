// UDP send build over pool buffers (rns_tx_udp_send_pool_dev): udp_send's datagrams, built on the device
// from the demux's records (or a host's own) into the pool transmit form.
// (The kernels of k_udp_tx.hip alone: they are no templates.  Their arguments are in rns_k_args.hpp.)
#pragma once

#include "rns_k_args.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// udp_send (udp.rs:101-114) copies the caller's bytes into fresh buffers (append_from_slice), udp_output
// (udp.rs:150-173) prepends the 8-byte UDP header (alloc_header) and checksums the packet, and ip_output_v4 /
// ip_output_v6 (ip.rs:133-177) write their header in front in the same head buffer.  Here a record of the
// UDP demux read as a send — to its address and port, from its socket's port — becomes that datagram in
// three launches on one stream, the echo responder's decomposition; grid-wide ordering comes from the
// launch boundaries only:
//   1. udp_tx_classify_kernel  a lane per record, a wave per 64 records, four waves per workgroup: reads the
//                              record's second half, applies the send test, finds the socket whose range of
//                              d_q_first holds the record (a binary search) and leaves one dword per record
//                              in the workspace (send, IPv4, payload buffers, the socket's port) and the
//                              workgroup's sums of (payload buffers, sends) and (IPv4 sends, 0).
//   2. scan2_parts_kernel      (rns_k_scan.hpp, through k_scan.hip) over each of the two sum arrays.
//   3. udp_tx_build_kernel     the same decomposition: scans its workgroup again, applies send_cap and the
//                              free list's length (both counts are monotone: the built sends are a prefix),
//                              then each wave walks the 16-byte chunks of all its payloads concatenated.
//                              A payload starts 16-byte aligned in d_data and at the start of a buffer in
//                              the pool: a chunk is one whole aligned load and one whole aligned store,
//                              a payload's last chunk with zeros after its bytes (the datagram's own buffer).
//                              The chunks' little-endian word sums are reduced per datagram across the lanes
//                              (wave_dgram_sum) into LDS.  The owner lane then folds in the UDP header and
//                              the pseudo-header and stores the head — both checksums filled — and the
//                              descriptors.  The payload is read once and written once.
// The counts are stored by one lane of the grid — the first send that is not built (its exclusive counts) or,
// when all are, the last send — into the zeroed d_count: no atomics.
// ---------------------------------------------------------------------------
constexpr uint32_t kUdpTxWaves = kScanBlock / 64;
// The wave's LDS table, a row of 64 per field: the wave's chunks before the datagram (place_owner's row), its
// payload's off16 and bytes, its first payload buffer's place in d_free, its payload's little-endian word sum.
constexpr int kUtBefore = kPdBefore, kUtOff = 1, kUtLen = 2, kUtFree = 3, kUtSum = 4, kUtRows = 5;

// the workspace's dword per record: send, IPv4, payload buffers (<= 256), the socket's port in the high half
constexpr uint32_t kUtRecSend = 1u, kUtRecV4 = 2u;
constexpr int kUtRecBufShift = 2, kUtRecPortShift = 16;
constexpr uint32_t kUtRecBufMask = 0x1ffu;

__global__ __launch_bounds__(kScanBlock) void udp_tx_classify_kernel(const UdpTxArgs a)
{
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    const bool live = k < a.n_recs;
    uint32_t rec = 0;
    if (live && k < a.q_first[a.n_socks]) {
        const uint4 r1 = a.rec_in[2 * k + 1];  // src, off16, sport | len << 16, family | flags << 8
        const uint32_t len = r1.z >> 16, fam = r1.w & 0xffu, flags = (r1.w >> 8) & 0xffu;
        if ((flags & RNS_UDP_QUEUED) && (fam == 4u || fam == 6u) && 16ull * r1.y + len <= a.data_bytes) {
            // the last socket whose first record is at or before k: at most 10 steps, every index below n_socks
            uint32_t lo = 0, hi = a.n_socks;
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (a.q_first[mid] <= k)
                    lo = mid;
                else
                    hi = mid;
            }
            rec = kUtRecSend | (fam == 4u ? kUtRecV4 : 0u) | (((len + (1u << a.blog) - 1u) >> a.blog) << kUtRecBufShift) |
                  (static_cast<uint32_t>(a.sock_port[lo]) << kUtRecPortShift);
        }
    }
    if (live)
        a.rec[k] = rec;
    uint2 ta, tb;
    (void)scan2_block(make_uint2((rec >> kUtRecBufShift) & kUtRecBufMask, rec & kUtRecSend), ta);
    (void)scan2_block(make_uint2((rec & kUtRecV4) ? 1u : 0u, 0u), tb);
    if (threadIdx.x == 0) {
        a.part_a[blockIdx.x] = ta;
        a.part_b[blockIdx.x] = tb;
    }
}

// One chunk of the wave's concatenated payloads: its 16 bytes (zeros after the payload's last byte) and where
// they go.
struct UdpTxChunk {
    uint4 x;
    uint8_t *dc;   // the chunk's 16-byte-aligned address in the transmit pool
    uint32_t hi;   // its payload bytes are [0, hi); 0: no chunk
    uint32_t j;    // its datagram's lane, ~0: no chunk
    uint32_t c;    // its index among its datagram's chunks
};

// Chunk v of the wave's W chunks, its load issued.  The send test found the payload's bytes inside d_data; a last
// chunk that is not whole inside d_data (a payload that ends in the last 15 bytes of a d_data whose size is no
// multiple of 16) is read byte by byte.
__device__ __forceinline__ UdpTxChunk udp_tx_chunk(const UdpTxArgs &a, const uint32_t (&pd)[kUtRows][64], uint32_t v, uint32_t W)
{
    UdpTxChunk ck{};
    ck.j = ~0u;
    if (v >= W)
        return ck;
    const uint32_t j = place_owner(pd, v);
    const uint32_t c = v - pd[kUtBefore][j], len = pd[kUtLen][j];
    const uint64_t at = 16ull * (static_cast<uint64_t>(pd[kUtOff][j]) + c);  // < data_bytes: byte 16 c of the payload
    if (a.data_bytes - at >= 16u) {
        ck.x = *reinterpret_cast<const uint4 *>(a.data + at);
    } else {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; ++b)
            if (at + b < a.data_bytes)
                w[b >> 2] |= static_cast<uint32_t>(a.data[at + b]) << (8 * (b & 3));
        ck.x = make_uint4(w[0], w[1], w[2], w[3]);
    }
    ck.hi = min(16u, len - 16u * c);  // >= 1: c is below the datagram's chunk count
    if (ck.hi != 16u) {
        const int hi = static_cast<int>(ck.hi);
        ck.x = make_uint4(keep_bytes(ck.x.x, 0, hi, 0), keep_bytes(ck.x.y, 0, hi, 4), keep_bytes(ck.x.z, 0, hi, 8),
                          keep_bytes(ck.x.w, 0, hi, 12));
    }
    // chunk c of a payload lies in buffer c >> (blog - 4); the datagram's buffers were found inside the transmit
    // pool before its chunks were counted
    const uint32_t bi = a.free[pd[kUtFree][j] + (c >> (a.blog - 4u))];
    ck.dc = a.tx_pool + (static_cast<uint64_t>(bi) << a.blog) + ((16u * c) & ((1u << a.blog) - 1u));
    ck.j = j;
    ck.c = c;
    return ck;
}

// Stores the chunk whole and adds its little-endian word sum to its datagram's in LDS.  (Called by the whole wave.)
__device__ __forceinline__ void udp_tx_emit(const UdpTxChunk &ck, uint32_t (&pd)[kUtRows][64], uint32_t lane)
{
    uint32_t sum = 0;
    if (ck.hi != 0) {
        *reinterpret_cast<uint4 *>(ck.dc) = ck.x;
        sum = sad4(ck.x, 0u);  // <= 8 * 0xffff
    }
    wave_dgram_sum(sum, ck.j, ck.c, ck.hi != 0, lane, pd[kUtSum]);
}

__global__ __launch_bounds__(kScanBlock) void udp_tx_build_kernel(const UdpTxArgs a)
{
    __shared__ uint32_t pds[kUdpTxWaves][kUtRows][64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t(&pd)[kUtRows][64] = pds[wv];
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    const bool live = k < a.n_recs;
    const uint32_t rec = live ? a.rec[k] : 0u;
    const bool snd = (rec & kUtRecSend) != 0, v4 = (rec & kUtRecV4) != 0;
    const uint32_t pbufs = (rec >> kUtRecBufShift) & kUtRecBufMask;
    uint2 ta, tb;
    const uint2 xa = scan2_block(make_uint2(pbufs, snd ? 1u : 0u), ta);
    const uint2 xb = scan2_block(make_uint2(v4 ? 1u : 0u, 0u), tb);
    const uint2 ca = a.part_a[blockIdx.x], cb = a.part_b[blockIdx.x];
    // exclusive counts before this record: sends, their buffers (64 bits), IPv4 sends
    const uint32_t r = ca.y + xa.y, v4_before = cb.x + xb.x;
    const uint64_t f0 = static_cast<uint64_t>(ca.x + xa.x) + r;
    const uint32_t nfr = 1u + pbufs;
    const bool built = snd && r < a.send_cap && f0 + nfr <= a.n_free;
    // the record, as the classify read it: the destination, then src, off16, sport | len << 16, family | flags << 8
    uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0;
    if (built) {
        r0 = a.rec_in[2 * k];
        r1 = a.rec_in[2 * k + 1];
    }
    const uint32_t len = r1.z >> 16;
    const uint32_t fi = static_cast<uint32_t>(f0);  // built: f0 < n_free
    bool bad = false;
    if (built) {
        for (uint32_t q = 0; q < nfr; ++q)
            bad = bad || a.free[fi + q] >= a.tx_bufs;
    }
    if (live)
        a.send[k] = static_cast<uint8_t>(!snd ? 0u : !built ? RNS_UDPTX_SEND | RNS_UDPTX_NOBUF
                                                  : bad    ? RNS_UDPTX_SEND | RNS_UDPTX_BADBUF
                                                           : RNS_UDPTX_SEND | RNS_UDPTX_BUILT);
    // the totals, stored by one lane of the grid: the first send that is not built holds them as its exclusive
    // counts (its predecessor was built: r - 1 < send_cap and f0 <= n_free), and when every send is built the
    // last one holds them as its inclusive counts.  (No send built: the zeroed d_count stands.)
    if (snd && (built ? r + 1u == a.part_a[gridDim.x].y : r != 0 && r - 1u < a.send_cap && f0 <= a.n_free)) {
        a.count[0] = r + (built ? 1u : 0u);
        a.count[1] = fi + (built ? nfr : 0u);
        a.count[2] = v4_before + (built && v4 ? 1u : 0u);
    }
    const uint64_t bm = __ballot(built);
    if (!bm)
        return;  // (after the workgroup's last barrier)
    // the wave's chunks, concatenated: at most 64 * 4096 of them, 128 at a time with both halves' loads in flight
    const bool copy = built && !bad;
    const uint32_t nck = copy ? (len + 15u) >> 4 : 0u;
    const uint32_t cinc = wave_incl_scan(nck);
    const uint32_t W = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cinc), 63));
    pd[kUtSum][lane] = 0u;
    if (W != 0) {
        pd[kUtBefore][lane] = cinc - nck;
        pd[kUtOff][lane] = r1.y;
        pd[kUtLen][lane] = len;
        pd[kUtFree][lane] = fi + 1u;
        wave_lds_fence();
        for (uint32_t vb = 0; vb < W; vb += 128u) {
            const UdpTxChunk c0 = udp_tx_chunk(a, pd, vb + lane, W);
            const UdpTxChunk c1 = udp_tx_chunk(a, pd, vb + 64u + lane, W);
            udp_tx_emit(c0, pd, lane);
            udp_tx_emit(c1, pd, lane);
        }
    }
    wave_lds_fence();
    if (!built)
        return;
    // the owner lane: the descriptors, then the head with both checksums
    a.tx_head_len8[r] = static_cast<uint8_t>(bad ? 0u : v4 ? 28u : 48u);
    a.tx_pay_len16[r] = static_cast<uint16_t>(len);
    if (a.tx_src)
        a.tx_src[r] = static_cast<uint32_t>(k);
    if ((r & 63u) == 0)
        a.tx_blk_first[r >> 6] = fi;
    if (bad)
        return;
    const uint32_t B = 1u << a.blog;
    uint8_t *const hb = a.tx_pool + (static_cast<uint64_t>(a.free[fi]) << a.blog) + B;
    const uint32_t pay_be = bswap16_u32(fold16(pd[kUtSum][lane]));  // the payload's big-endian word sum, folded (RFC 1071 2(B))
    // udp_output: source port, destination port, length as u16, checksum over the pseudo-header and the packet
    const uint32_t sport = rec >> kUtRecPortShift, dport = r1.z & 0xffffu, ulen = (8u + len) & 0xffffu;
    const uint32_t ports = bswap16_u32(sport) | (bswap16_u32(dport) << 16);
    const uint32_t l4 = 17u + ulen + sport + dport + ulen + pay_be;  // without the addresses
    if (v4) {
        // ip_output_v4: 45 00 len | id 0000 | 40 11 csum | local | destination
        const uint32_t total = (28u + len) & 0xffffu;
        const uint32_t id = (a.ip_id_base + (a.ip_id_add ? *a.ip_id_add : 0u) + v4_before) & 0xffffu;
        const uint32_t addrs = be2(a.local4) + be2(r0.x);
        const uint32_t ipck = fold16(0x4500u + total + id + 0x4011u + addrs) ^ 0xffffu;
        const uint32_t ck = fold16(l4 + addrs) ^ 0xffffu;  // a computed 0 is stored as 0
        uint8_t *const at = hb - 28u;  // 4 mod 16
        *reinterpret_cast<uint32_t *>(at) = 0x45u | (bswap16_u32(total) << 16);
        *reinterpret_cast<uint2 *>(at + 4) = make_uint2(bswap16_u32(id), 0x1140u | (bswap16_u32(ipck) << 16));
        *reinterpret_cast<uint4 *>(at + 12) = make_uint4(a.local4, r0.x, ports, bswap16_u32(ulen) | (bswap16_u32(ck) << 16));
    } else {
        // ip_output_v6: 60 00 00 00 | len 11 40 | local | destination
        uint32_t s = l4;
        s += be2(a.local6[0]) + be2(a.local6[1]) + be2(a.local6[2]) + be2(a.local6[3]);
        s += be2(r0.x) + be2(r0.y) + be2(r0.z) + be2(r0.w);
        const uint32_t ck = fold16(s) ^ 0xffffu;
        uint8_t *const at = hb - 48u;  // 0 mod 16
        *reinterpret_cast<uint4 *>(at) = make_uint4(0x60u, bswap16_u32(ulen) | (17u << 16) | (64u << 24), a.local6[0], a.local6[1]);
        *reinterpret_cast<uint4 *>(at + 16) = make_uint4(a.local6[2], a.local6[3], r0.x, r0.y);
        *reinterpret_cast<uint4 *>(at + 32) = make_uint4(r0.z, r0.w, ports, bswap16_u32(ulen) | (bswap16_u32(ck) << 16));
    }
}

}  // namespace rns
