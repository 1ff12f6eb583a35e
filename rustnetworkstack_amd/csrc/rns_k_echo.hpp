// ICMP echo responder over pool buffers (rns_rx_icmp_echo_pool_dev): icmp_input's reply, built on the
// device from a verified receive batch into the pool transmit form.
// (The kernels of k_echo.hip alone: two of them are no templates.  Their arguments are in rns_k_args.hpp.)
#pragma once

#include "rns_k_args.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// icmp_input_v4 / icmp_input_v6 (icmp.rs:44-85) verify the request, copy its payload into fresh
// buffers (append_from_buffer), prepend a zeroed 4-byte ICMP header (alloc_header), checksum the
// reply and hand it to ip_output, which writes its header in front in the same head buffer.  Here
// the pool verify runs as it is, then three more steps on the same stream; grid-wide ordering comes
// from the launch boundaries only:
//   1. echo_classify_kernel  a lane per datagram, a wave per 64-datagram block (the unit of
//                            d_blk_first), four blocks per workgroup: reads the status and the first
//                            buffer's header dwords, decides the request, leaves one dword per
//                            datagram in the workspace (request, IPv4, payload buffers, IHL) and the
//                            workgroup's sums of (payload buffers, requests) and (IPv4 requests, 0).
//   2. scan2_parts_kernel    (rns_k_scan.hpp, through k_scan.hip) over each of the two sum arrays.
//                            The buffers before a request are payload buffers + requests, added in
//                            64 bits.
//   3. echo_build_kernel     the same decomposition: allocates the replies' buffers (tx_alloc,
//                            rns_k_pool_txform.hpp), then each wave walks the destination 16-byte
//                            chunks of all its replies concatenated (pool_walk, rns_k_pool_view.hpp),
//                            the destination in the reply's payload buffers, which start 16-byte aligned:
//                            every chunk is one whole aligned store, a payload's last chunk with
//                            zeros after its bytes (the reply's own buffer).  The chunks' little-endian
//                            word sums are reduced per datagram across the lanes (a range of the wave's
//                            prefix sum: a datagram's chunks are consecutive lanes) into LDS; chunks start at even
//                            payload offsets, so the sums add whatever the position.  The owner lane
//                            then folds in the head and the IPv6 pseudo-header, and stores the head —
//                            both checksums filled — and the descriptors.  The payload is read once and
//                            written once after the verify.
// The allocation, the counts, the status bits and the descriptors are the pool transmit form's
// (rns_k_pool_txform.hpp), shared with the UDP send build; the IP head words are composed there too.
// ---------------------------------------------------------------------------
constexpr uint32_t kEchoWaves = kScanBlock / 64;
// The wave's LDS table: pool_walk's rows, then an answered request's first payload buffer's place in d_free
// and the little-endian word sum of its payload.
constexpr int kEchoPd = kPdRows + 2, kEchoPdFree = kPdRows, kEchoPdSum = kPdRows + 1;

// the workspace's dword per datagram
constexpr uint32_t kEchoRecReq = 1u, kEchoRecV4 = 2u;
constexpr int kEchoRecBufShift = 2, kEchoRecIhlShift = 12;  // payload buffers (<= 256), ip_hdr / 4 (<= 15)

__global__ __launch_bounds__(kScanBlock) void echo_classify_kernel(const EchoArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t blk = blockIdx.x * kEchoWaves + (threadIdx.x >> 6);
    const PoolLane e = pool_lane(a.rx, blk, lane);
    const uint32_t stv = e.live ? a.rx.status[e.p] : 0u;
    // the first buffer's checks (rns_k_pool_view.hpp says why each read is safe), as this kernel's own lines
    bool ok = e.live && (stv & RNS_RX_ACCEPT) && e.nf != 0 && e.gi + e.nf <= a.rx.n_frags;
    uint32_t rec = 0;
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
            // the ICMP header's dword lies in the first buffer (ip_hdr + 4 <= 64 <= B) and inside the datagram
            if (ip_hdr + 4u <= e.T && proto == (v6 ? 58u : 1u) && (h[ip_hdr >> 2] & 0xffu) == (v6 ? 128u : 8u)) {
                const uint32_t pay = e.T - ip_hdr - 4u;
                rec = kEchoRecReq | (v6 ? 0u : kEchoRecV4) | (((pay + (1u << a.rx.blog) - 1u) >> a.rx.blog) << kEchoRecBufShift) |
                      ((ip_hdr >> 2) << kEchoRecIhlShift);
            }
        }
    }
    if (e.live)
        a.w.rec[e.p] = rec;
    build_parts(a.w, (rec >> kEchoRecBufShift) & 0x3ffu, rec & kEchoRecReq, (rec & kEchoRecV4) != 0);
}

// Stores the chunk whole (zeros after a payload's last byte) and adds its little-endian word sum to its
// datagram's in LDS (wave_dgram_sum, rns_k_pool_view.hpp, which the UDP send build shares).  (Called by the
// whole wave.)
__device__ __forceinline__ void echo_emit(const PlaceChunk &ck, const uint4 y, uint32_t (&pd)[kEchoPd][64], uint32_t lane)
{
    uint32_t sum = 0;
    if (ck.hi != 0) {
        uint32_t o[4];
        place_join(ck, y, o);
        if (ck.hi != 16u) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                o[k] = keep_bytes(o[k], 0, static_cast<int>(ck.hi), 4 * k);
        }
        *reinterpret_cast<uint4 *>(ck.dc) = make_uint4(o[0], o[1], o[2], o[3]);
        sum = sad4(make_uint4(o[0], o[1], o[2], o[3]), 0u);  // <= 8 * 0xffff
    }
    wave_dgram_sum(sum, ck.j, ck.c, ck.hi != 0, lane, pd[kEchoPdSum]);
}

template <bool NT>
__global__ __launch_bounds__(kScanBlock) void echo_build_kernel(const EchoArgs a)
{
    __shared__ uint32_t pds[kEchoWaves][kEchoPd][64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t(&pd)[kEchoPd][64] = pds[wv];
    const uint32_t blk = blockIdx.x * kEchoWaves + wv;
    const PoolLane e = pool_lane(a.rx, blk, lane);
    const uint32_t rec = e.live ? a.w.rec[e.p] : 0u;
    const bool req = (rec & kEchoRecReq) != 0, v4 = (rec & kEchoRecV4) != 0;
    const uint32_t pbufs = (rec >> kEchoRecBufShift) & 0x3ffu, ip_hdr = ((rec >> kEchoRecIhlShift) & 0xfu) * 4u;
    const TxSlot t = tx_alloc(a.tx, a.w, req, pbufs, v4, [](bool) {});
    const uint32_t pay = req ? e.T - ip_hdr - 4u : 0u;
    if (e.live)
        a.echo[e.p] = tx_status(t, req);
    const uint64_t bm = __ballot(t.built);
    if (!bm)
        return;  // (after the workgroup's last barrier)
    // the wave's destination chunks, concatenated: at most 64 * 4096 of them
    const bool copy = t.built && !t.bad;
    const uint32_t nck = copy ? (pay + 15u) >> 4 : 0u;
    const uint32_t cinc = wave_incl_scan(nck);
    const uint32_t W = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cinc), 63));
    pd[kEchoPdSum][lane] = 0u;
    if (W != 0) {
        pool_rows(pd, lane, cinc - nck, e.gi, ip_hdr + 4u, pay);
        pd[kEchoPdFree][lane] = t.fi + 1u;
        wave_lds_fence();
        pool_walk<NT>(
            a.rx, pd, W, lane,
            [](uint32_t) { return 0u; },
            [&](uint32_t j, uint32_t c) { return tx_chunk_dst(a.tx, pd[kEchoPdFree][j], c); },
            [&](const PlaceChunk &ck, const uint4 y) { echo_emit(ck, y, pd, lane); });
    }
    wave_lds_fence();
    if (!t.built)
        return;
    // the owner lane: the descriptors, then the head with both checksums
    uint8_t *const hb = tx_describe(a.tx, t, v4 ? 24u : 44u, pay, e.p);
    if (t.bad)
        return;
    const uint32_t *h = pool_first(a.rx, e);  // a request: the classify found it inside the pool
    const uint32_t pay_be = bswap16_u32(fold16(pd[kEchoPdSum][lane]));  // the payload's big-endian word sum, folded (RFC 1071 2(B))
    if (v4) {
        // ip_output_v4, protocol 1, to the requester; then 00 00 csum (icmp_output)
        const Ip4Head ip = ip4_head(24u + pay, ip_id(a.tx.ip_id_base, a.tx.ip_id_add, t.v4_before), 1u, a.local.v4, h[3]);
        const uint32_t ck = pay_be ^ 0xffffu;  // seed 0, a head of zeros
        uint8_t *const at = hb - 24u;  // 8 mod 16
        *reinterpret_cast<uint2 *>(at) = make_uint2(ip.d[0], ip.d[1]);
        *reinterpret_cast<uint4 *>(at + 8) = make_uint4(ip.d[2], ip.d[3], ip.d[4], bswap16_u32(ck) << 16);
    } else {
        // ip_output_v6, next header 58, to the requester; then 81 00 csum
        const uint32_t plen = 4u + pay;
        const uint32_t peer[4] = {h[2], h[3], h[4], h[5]};
        const Ip6Head ip = ip6_head(plen, 58u, a.local.v6, peer);
        const uint32_t ck = fold16(plen + 58u + 0x8100u + pay_be + addr_sum6(a.local.v6, peer)) ^ 0xffffu;
        uint8_t *const at = hb - 44u;  // 4 mod 16
        *reinterpret_cast<uint32_t *>(at) = ip.d[0];
        *reinterpret_cast<uint2 *>(at + 4) = make_uint2(ip.d[1], ip.d[2]);
        *reinterpret_cast<uint4 *>(at + 12) = make_uint4(ip.d[3], ip.d[4], ip.d[5], ip.d[6]);
        *reinterpret_cast<uint4 *>(at + 28) = make_uint4(ip.d[7], ip.d[8], ip.d[9], 0x81u | (bswap16_u32(ck) << 16));
    }
}

}  // namespace rns
