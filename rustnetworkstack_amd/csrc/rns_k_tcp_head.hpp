// The byte-order helpers and the one builder of a TCP/IPv4 or TCP/IPv6 head out of a per-flow template
// (rule, patch, checksum sums, store) that the segmentation, the ACK build, the control-segment build and the
// send planning share.
// Plain integer C++, no wave intrinsics, no LDS: a host compiler takes it (tests/cpp/test_tcp_head.cpp).
// (The first part of rns_kernels.hpp: it builds on nothing.)
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define RNS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RNS_HD inline
#endif

namespace rns {

RNS_HD uint32_t bswap16_u32(uint32_t x) { return ((x & 0xff) << 8) | (x >> 8); }  // x <= 0xffff

// Two big-endian 16-bit words of a dword held little-endian (bytes b0 b1 b2 b3): b0b1 + b2b3.
RNS_HD uint32_t be2(uint32_t d)
{
    const uint32_t x = ((d & 0x00ff00ffu) << 8) | ((d >> 8) & 0x00ff00ffu);
    return (x & 0xffffu) + (x >> 16);
}

RNS_HD uint32_t fold16(uint32_t x)
{
    while (x > 0xffff)
        x = (x & 0xffff) + (x >> 16);
    return x;
}

// The template rule of the ACK build and the send planning: a head of hl = 40 (IPv4) or 60 (IPv6)
// bytes inside its row, the version and the protocol TCP's, no TCP options.  (The segmentation takes
// options and heads of up to 100 bytes: its wider rule is its own.)
RNS_HD bool tcp_tmpl_ok(const uint8_t *t, uint32_t hl, uint32_t tmpl_stride)
{
    if ((hl != 40u && hl != 60u) || hl > tmpl_stride)
        return false;
    const bool v4 = hl == 40u;
    const uint32_t b0 = t[0], iphdr = v4 ? 20u : 40u;
    return (v4 ? b0 == 0x45u && t[9] == 6u : (b0 >> 4) == 6u && t[6] == 6u) && (t[iphdr + 12u] >> 4) == 5u;
}

// Dword k of a head from the template's dword d (send_packet, tcp_output, ip_output): the IPv4 id,
// seq, ack and the data offset | flags | window dword; ipd = the IP header's dwords.  fin = the head
// is final: the length fields for pay payload bytes (40 + pay <= 0xffff) are written and both checksum
// fields zeroed, as the ACK build needs them; the planning leaves both to the segmentation.
RNS_HD uint32_t tcp_head_patch(uint32_t k, uint32_t d, bool v4, uint32_t ipd, uint32_t id, uint32_t seq, uint32_t ack,
                               uint32_t window, uint32_t flags, bool fin, uint32_t pay = 0)
{
    if (v4 && k == 1u)  // ip.rs:147: id
        d = (d & 0xffff0000u) | bswap16_u32(id);
    if (fin) {
        if (v4 && k == 0u)  // ip.rs:146: total length
            d = (d & 0xffffu) | (bswap16_u32(40u + pay) << 16);
        if (v4 && k == 2u)
            d &= 0xffffu;
        if (!v4 && k == 1u)  // ip.rs:170: payload length
            d = (d & 0xffff0000u) | bswap16_u32(20u + pay);
        if (k == ipd + 4u)
            d &= 0xffff0000u;
    }
    if (k == ipd + 1u)  // tcp.rs:947-951
        d = __builtin_bswap32(seq);
    if (k == ipd + 2u)
        d = __builtin_bswap32(ack);
    if (k == ipd + 3u)
        d = 0x50u | (flags << 8) | (bswap16_u32(window) << 16);
    return d;
}

// The big-endian word sums of a head's dwords, both checksum fields zero: the IP header's, the
// addresses' (the pseudo-header's part of it) and the TCP header's.
struct TcpHeadSum {
    uint32_t ip = 0, tcp = 0, addr = 0;

    RNS_HD void add(uint32_t k, uint32_t d, bool v4, uint32_t ipd)
    {
        const uint32_t b = be2(d);
        ip += k < ipd ? b : 0u;
        tcp += k < ipd ? 0u : b;
        addr += (k >= (v4 ? 3u : 2u) && k < ipd) ? b : 0u;
    }
    RNS_HD uint32_t ip_csum() const { return fold16(ip) ^ 0xffffu; }  // the IPv4 header checksum (ip.rs:158-159)
    // The folded sum, in [1, 0xffff], of the pseudo-header (tcp.rs:957-966) for tcplen = TCP header + payload
    // bytes and of the TCP header: the TCP checksum is its complement once the payload's sum is folded on.
    RNS_HD uint32_t l4_head(uint32_t tcplen) const
    {
        const uint32_t t1 = fold16(addr + 6u + (tcplen & 0xffffu)) + fold16(tcp);
        return (t1 & 0xffffu) + (t1 >> 16);
    }
};

// A final control segment's head (no options, no payload: a pure ACK, a FIN, an RST) out of the template t
// that tcp_tmpl_ok passed, to the 4-byte aligned o: hl = 40 (v4) / 60 bytes, both checksums filled (tcp.rs:957-973,
// ip.rs:158-159).  One pass: every dword but the two that hold a checksum is stored as it is summed.
RNS_HD void tcp_ctl_head_store(uint32_t *o, const uint8_t *t, bool v4, uint32_t hl, uint32_t id, uint32_t seq, uint32_t ack, uint32_t window,
                               uint32_t flags)
{
    const uint32_t ipd = v4 ? 5u : 10u, nd = hl >> 2;
    const uint32_t kip = v4 ? 2u : ~0u, kl4 = ipd + 4u;
    uint32_t dip = 0, dl4 = 0;
    TcpHeadSum hs;
    for (uint32_t j = 0; j < nd; ++j) {
        uint32_t d;
        __builtin_memcpy(&d, t + 4u * j, 4);
        d = tcp_head_patch(j, d, v4, ipd, id, seq, ack, window, flags, true);
        hs.add(j, d, v4, ipd);
        if (j == kip)
            dip = d;
        else if (j == kl4)
            dl4 = d;
        else
            o[j] = d;
    }
    if (v4)
        o[2] = dip | (bswap16_u32(hs.ip_csum()) << 16);
    o[kl4] = dl4 | bswap16_u32(hs.l4_head(20u) ^ 0xffffu);
}

// Dword d to o at any alignment: one dword store when o is 4-byte aligned (al4), bytes otherwise.  (The
// segmentation's per-lane write-back keeps its own two loops: through this function the hot kernel's
// code grew and its registers were allocated anew.)
RNS_HD void store_dword(uint8_t *o, uint32_t d, bool al4)
{
    if (al4) {
        *reinterpret_cast<uint32_t *>(o) = d;
    } else {
        o[0] = static_cast<uint8_t>(d);
        o[1] = static_cast<uint8_t>(d >> 8);
        o[2] = static_cast<uint8_t>(d >> 16);
        o[3] = static_cast<uint8_t>(d >> 24);
    }
}

}  // namespace rns
