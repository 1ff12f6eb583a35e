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
//   3. udp_tx_build_kernel     the same decomposition: allocates the datagrams' buffers (tx_alloc,
//                              rns_k_pool_txform.hpp), then each wave walks the 16-byte chunks of all its
//                              payloads concatenated.
//                              A payload starts 16-byte aligned in d_data and at the start of a buffer in
//                              the pool: a chunk is one whole aligned load and one whole aligned store,
//                              a payload's last chunk with zeros after its bytes (the datagram's own buffer).
//                              The chunks' little-endian word sums are reduced per datagram across the lanes
//                              (wave_dgram_sum) into LDS.  The owner lane then folds in the UDP header and
//                              the pseudo-header and stores the head — both checksums filled — and the
//                              descriptors.  The payload is read once and written once.
// The allocation, the counts, the status bits and the descriptors are the pool transmit form's
// (rns_k_pool_txform.hpp), shared with the echo responder; the IP head words are composed there too.
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
            rec = kUtRecSend | (fam == 4u ? kUtRecV4 : 0u) | (((len + (1u << a.tx.blog) - 1u) >> a.tx.blog) << kUtRecBufShift) |
                  (static_cast<uint32_t>(a.sock_port[lo]) << kUtRecPortShift);
        }
    }
    if (live)
        a.w.rec[k] = rec;
    build_parts(a.w, (rec >> kUtRecBufShift) & kUtRecBufMask, rec & kUtRecSend, (rec & kUtRecV4) != 0);
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
    ck.dc = tx_chunk_dst(a.tx, pd[kUtFree][j], c);
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
    const uint32_t rec = live ? a.w.rec[k] : 0u;
    const bool snd = (rec & kUtRecSend) != 0, v4 = (rec & kUtRecV4) != 0;
    // the record, as the classify read it: the destination, then src, off16, sport | len << 16, family | flags << 8
    uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0;
    const TxSlot t = tx_alloc(a.tx, a.w, snd, (rec >> kUtRecBufShift) & kUtRecBufMask, v4, [&](bool built) {
        if (built) {
            r0 = a.rec_in[2 * k];
            r1 = a.rec_in[2 * k + 1];
        }
    });
    const uint32_t len = r1.z >> 16;
    if (live)
        a.send[k] = tx_status(t, snd);
    const uint64_t bm = __ballot(t.built);
    if (!bm)
        return;  // (after the workgroup's last barrier)
    // the wave's chunks, concatenated: at most 64 * 4096 of them, 128 at a time with both halves' loads in flight
    const bool copy = t.built && !t.bad;
    const uint32_t nck = copy ? (len + 15u) >> 4 : 0u;
    const uint32_t cinc = wave_incl_scan(nck);
    const uint32_t W = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cinc), 63));
    pd[kUtSum][lane] = 0u;
    if (W != 0) {
        pd[kUtBefore][lane] = cinc - nck;
        pd[kUtOff][lane] = r1.y;
        pd[kUtLen][lane] = len;
        pd[kUtFree][lane] = t.fi + 1u;
        wave_lds_fence();
        for (uint32_t vb = 0; vb < W; vb += 128u) {
            const UdpTxChunk c0 = udp_tx_chunk(a, pd, vb + lane, W);
            const UdpTxChunk c1 = udp_tx_chunk(a, pd, vb + 64u + lane, W);
            udp_tx_emit(c0, pd, lane);
            udp_tx_emit(c1, pd, lane);
        }
    }
    wave_lds_fence();
    if (!t.built)
        return;
    // the owner lane: the descriptors, then the head with both checksums
    uint8_t *const hb = tx_describe(a.tx, t, v4 ? 28u : 48u, len, k);
    if (t.bad)
        return;
    const uint32_t pay_be = bswap16_u32(fold16(pd[kUtSum][lane]));  // the payload's big-endian word sum, folded (RFC 1071 2(B))
    // udp_output: source port, destination port, length as u16, checksum over the pseudo-header and the packet
    const uint32_t sport = rec >> kUtRecPortShift, dport = r1.z & 0xffffu, ulen = (8u + len) & 0xffffu;
    const uint32_t ports = bswap16_u32(sport) | (bswap16_u32(dport) << 16);
    const uint32_t l4 = 17u + ulen + sport + dport + ulen + pay_be;  // without the addresses
    if (v4) {
        // ip_output_v4, protocol 17, to the record's address
        const Ip4Head ip = ip4_head(28u + len, ip_id(a.tx.ip_id_base, a.tx.ip_id_add, t.v4_before), 17u, a.local.v4, r0.x);
        const uint32_t ck = fold16(l4 + addr_sum4(a.local.v4, r0.x)) ^ 0xffffu;  // a computed 0 is stored as 0
        uint8_t *const at = hb - 28u;  // 4 mod 16
        *reinterpret_cast<uint32_t *>(at) = ip.d[0];
        *reinterpret_cast<uint2 *>(at + 4) = make_uint2(ip.d[1], ip.d[2]);
        *reinterpret_cast<uint4 *>(at + 12) = make_uint4(ip.d[3], ip.d[4], ports, bswap16_u32(ulen) | (bswap16_u32(ck) << 16));
    } else {
        // ip_output_v6, next header 17, to the record's address
        const uint32_t peer[4] = {r0.x, r0.y, r0.z, r0.w};
        const Ip6Head ip = ip6_head(ulen, 17u, a.local.v6, peer);
        const uint32_t ck = fold16(l4 + addr_sum6(a.local.v6, peer)) ^ 0xffffu;
        uint8_t *const at = hb - 48u;  // 0 mod 16
        *reinterpret_cast<uint4 *>(at) = make_uint4(ip.d[0], ip.d[1], ip.d[2], ip.d[3]);
        *reinterpret_cast<uint4 *>(at + 16) = make_uint4(ip.d[4], ip.d[5], ip.d[6], ip.d[7]);
        *reinterpret_cast<uint4 *>(at + 32) = make_uint4(ip.d[8], ip.d[9], ports, bswap16_u32(ulen) | (bswap16_u32(ck) << 16));
    }
}

}  // namespace rns
