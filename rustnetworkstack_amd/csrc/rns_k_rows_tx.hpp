// Transmit finalize through the rows: the transmit parse helpers, the owner's finish (tx_finish), the
// field store and csum_rows_tx_kernel.
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_rows_rx.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// Transmit finalize through the rows decomposition (rns_tx_fill_packed_dev, round 6):
// tcp_output (tcp.rs:957-973), udp_output (udp.rs:151-171), icmp_output_v4/v6
// (icmp.rs:87-112) and ip_output_v4 (ip.rs:140-160) over a packed arena of finished
// datagrams.  The datagram's word sum T comes from the rows as in csum_rows_rx_kernel, and
// its owner holds the first 3 chunks (loaded a group of rows ahead of the row that streams
// them) — the IPv4 header without options, both fields of an IPv4 datagram, both addresses
// of either family; chunks 3-4 are loaded only by the owners that need them (IPv4 options,
// TCP over IPv6).  The owner parses the header, takes the header sum H and the two fields'
// bytes out of T (both fields count as zero: buf.rs:286-288), forms the pseudo-header from
// the header's own addresses and stores each result with one 2-byte store (two-byte stores
// measured no dearer than sector rewrites: profiles/r04_fill_store_ab.json).  The stash
// kernel this replaces needed a class pass, an LDS stash and two 32-byte sector rewrites.
// ---------------------------------------------------------------------------
#ifndef RNS_ROWS_TX_OCC  // waves/SIMD bound of the transmit form
#define RNS_ROWS_TX_OCC 6
#endif
#ifndef RNS_ROWS_TX_FIELD_AUX  // cache-policy bits of the packed finalize's field stores: plain (c3 305.2 /
#define RNS_ROWS_TX_FIELD_AUX 0  // IMIX 809.8 us; nontemporal 322.1 / 836.1, sc0|sc1 310.5 / 820.8: r06w)
#endif
constexpr uint32_t kNoField = 0xFFFFFFFFu;

// The first 40 bytes of a datagram (version, IHL, protocol and both addresses of either
// family) as ten dwords in datagram byte order, from its chunks (s = start & 15; chunk 0 is
// the 16-byte boundary at or below the start; s > 0 needs NS >= 4).
template <int NS>
__device__ __forceinline__ void head40(const uint4 (&ch)[NS], uint32_t s, uint32_t (&h)[10])
{
    uint32_t w[4 * NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        w[4 * c] = ch[c].x;
        w[4 * c + 1] = ch[c].y;
        w[4 * c + 2] = ch[c].z;
        w[4 * c + 3] = ch[c].w;
    }
    if (s == 0) {
#pragma unroll
        for (int k = 0; k < 10; ++k)
            h[k] = w[k];
        return;
    }
    if constexpr (NS >= 4) {
        const uint32_t q = s >> 2, sh = s & 3;
        uint32_t d[11];
#pragma unroll
        for (int k = 0; k < 11; ++k)
            d[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
#pragma unroll
        for (int k = 0; k < 10; ++k)
            h[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
    }
}

// The transmit path's reading of a datagram of L bytes whose first 40 bytes are h (head40)
// and whose IP header must lie within its first hl bytes: the IP header length, the L4 field
// (offset after the IP header: TCP 16, UDP 6, ICMPv4 / ICMPv6 2; kNoField for a protocol the
// stack does not checksum) and the pseudo-header sum the L4 output routine seeds with
// (tcp.rs:957-966, udp.rs:158-165, icmp.rs:97-104; none for ICMPv4, icmp.rs:87-95).  False:
// a datagram the stack cannot produce (bad version, IHL < 5, header past hl).
__device__ __forceinline__ bool tx_parse(const uint32_t (&h)[10], uint32_t L, uint32_t hl, uint32_t &hdr,
                                         uint32_t &field, uint32_t &seed, bool &v4)
{
    const uint32_t b0 = h[0] & 0xffu, version = b0 >> 4;
    uint32_t proto, addr;  // addr: BE word sum of source + destination (tcp.rs:958-966)
    if (version == 4) {
        hdr = (b0 & 15u) * 4u;
        if (hdr < 20 || hdr > hl)
            return false;
        proto = (h[2] >> 8) & 0xffu;            // header[9]
        addr = be2(h[3]) + be2(h[4]);            // header[12..20]
    } else if (version == 6) {
        hdr = 40;
        if (hl < 40)
            return false;
        proto = (h[1] >> 16) & 0xffu;           // header[6]
        addr = 0;
#pragma unroll
        for (int k = 2; k < 10; ++k)             // header[8..40]
            addr += be2(h[k]);
    } else {
        return false;
    }
    v4 = version == 4;
    const uint32_t seg = L - hdr, l16 = seg & 0xffffu;  // packet.len() as u16 (tcp.rs:942, udp.rs:152)
    field = kNoField;
    seed = 0;
    if (proto == 6 || proto == 17) {
        field = proto == 6 ? 16u : 6u;
        seed = fold16(addr + proto + l16);
    } else if (proto == 1 && v4) {
        field = 2;  // icmp_output_v4: no pseudo-header
    } else if (proto == 58 && !v4) {
        field = 2;  // icmp_output_v6: full length, protocol 58
        seed = fold16(addr + 58 + (seg >> 16) + (seg & 0xffffu));
    }
    return true;
}

// Owner-lane finish of transmit finalize for one datagram of L bytes: ch = its chunks from
// the 16-byte boundary at or below its start (raw memory bytes; s = start & 15; NS chunks
// hold bytes up to s + 78: the TCP field behind a 60-byte IPv4 header), mine = the
// datagram's word sum T (LE words at absolute pairing; L <= 65535, so no u32 wrap), odd =
// start & 1.  Exactly the stash kernel's transmit finish (csum_mixed_kernel, TX mode) and
// oracle.tx_fill_ref: fld[0] = 10 for IPv4 (ip_output_v4 over IHL*4 bytes), fld[1] = the
// L4 field (TCP 16, UDP 6, ICMPv4 / ICMPv6 2, after the IP header) when the segment holds
// it; val[] = the values to store big-endian (complemented; UDP's 0 stored as is).
template <int NS>
__device__ __forceinline__ uint8_t tx_finish(const uint4 (&ch)[NS], uint32_t mine, uint32_t s, uint32_t L, bool odd,
                                             bool present, uint32_t (&fld)[2], uint32_t (&val)[2])
{
    fld[0] = fld[1] = kNoField;
    val[0] = val[1] = 0;
    if (!present)
        return RNS_TX_MALFORMED;
    uint32_t h[10];
    head40(ch, s, h);
    uint32_t hdr, field, seed;
    bool v4;
    if (!tx_parse(h, L, L, hdr, field, seed, v4))
        return RNS_TX_MALFORMED;
    const uint32_t seg = L - hdr;
    const int lo = static_cast<int>(s);
    const uint32_t H = stash_sum_le(ch, lo, lo + static_cast<int>(hdr));
    uint8_t st = 0;
    if (v4) {  // compute_checksum(header) with header[10..12] as zero
        fld[0] = 10;
        val[0] = finalize_bits(H - stash_sum_le(ch, lo + 10, lo + 12), odd, false, 0u, true, RNS_FLAG_COMPLEMENT);
        st |= RNS_TX_IP_FILLED;
    }
    if (field != kNoField && seg >= field + 2) {
        const uint32_t f = hdr + field;
        fld[1] = f;
        const uint32_t l4 = mine - H - stash_sum_le(ch, lo + static_cast<int>(f), lo + static_cast<int>(f) + 2);
        val[1] = finalize_bits(l4, odd, false, seed, true, RNS_FLAG_COMPLEMENT);
        st |= RNS_TX_L4_FILLED;
    }
    return st;
}

// set_be16 of a finished field at absolute arena offset fp (util.rs:132-135); AUX = the buffer
// store's cache-policy bits
template <bool BUF, int AUX = 0>
__device__ __forceinline__ void store_field(const CsumArgs &a, __amdgpu_buffer_rsrc_t rsrc, uint64_t fp, uint32_t v)
{
    uint8_t *w8 = const_cast<uint8_t *>(a.arena);
    if (fp & 1) {
        w8[fp] = static_cast<uint8_t>(v >> 8);
        w8[fp + 1] = static_cast<uint8_t>(v);
    } else if constexpr (BUF) {
        __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(bswap16_u32(v & 0xffffu)), rsrc,
                                              static_cast<uint32_t>(fp), 0, AUX);
    } else {
        *reinterpret_cast<uint16_t *>(w8 + fp) = static_cast<uint16_t>(bswap16_u32(v & 0xffffu));
    }
}

// (Rewriting each field's whole 64-byte memory segment from the owner's chunks where the segment
// lies inside the datagram — full-segment writes instead of partial ones, which the store probe
// measured cheaper on cold lines — was slower: c3 322.6-323.0 / IMIX 823.4-826.7 us against
// 305.8-306.6 / 810.7-812.8, parity green; it reloads chunks 3-5 after the rows: session r06e.)
template <bool NT, bool BUF, int D>
__global__ __launch_bounds__(64, D >= 16 ? 4 : RNS_ROWS_TX_OCC) void csum_rows_tx_kernel(const CsumArgs a)
{
    constexpr int kNS = 5;  // chunks 0-4: bytes 0..79 of a 16-byte-aligned datagram
    const uint32_t lane = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.arena), static_cast<short>(0), static_cast<int>(BUF ? buf_records(a) : 0), 0x00020000);
    const uint64_t recs = buf_records(a);
    const PackedUnit u = packed_unit(a, lane);
    const uint64_t p = u.p, r0 = u.r0, start = u.start();
    const uint32_t len = u.len, excl = u.excl, total = u.total;
    const bool live = u.live, ok = u.ok(a);
    const bool present = live && ok && len != 0;
    uint32_t mine = 0;
    uint8_t st = RNS_TX_MALFORMED;
    uint32_t fld[2], val[2];
    // the bytes a datagram's finish reads past chunk 2 (from its first chunk): IPv4 options
    // past byte 48, or an L4 field ending past it (TCP over IPv6, TCP / UDP behind options)
    auto need_bytes = [&](const uint4 c0) -> uint32_t {
        const uint32_t b0 = c0.x & 0xffu, v = b0 >> 4;
        const uint32_t proto = v == 4 ? (c0.z >> 8) & 0xffu : (c0.y >> 16) & 0xffu;
        const uint32_t hdr = v == 4 ? (b0 & 15u) * 4u : 40u;
        const uint32_t fend = hdr + (proto == 6 ? 18u : proto == 17 ? 8u : 4u);
        return v == 4 || v == 6 ? max(hdr, fend) : 0u;
    };
    if ((r0 & 15) == 0) {
        uint4 own[kNS];
#pragma unroll
        for (int i = 3; i < kNS; ++i)
            own[i] = make_uint4(0, 0, 0, 0);
        if (!__ballot(len > 64)) {
            // ---- ACK-sized unit: every owner takes its datagram whole ----
            mine = ack_unit_sum<BUF, false>(a, rsrc, recs, start, len, own);  // (the finish reads the raw chunks)
        } else {
            // ---- the rows: T, and the owner's first 3 chunks loaded a group ahead ----
            const uint32_t c0 = excl >> 4;
            const uint32_t e = len ? (excl + len - 1) >> 4 : c0;
            mine = rows_region_sum<NT, BUF, D, 3>(a, rsrc, recs, r0, total, c0, e, len, own);
            const uint32_t nb = present ? need_bytes(own[0]) : 0u;
            if (__ballot(nb > 48)) {
                own[3] = nb > 48 ? own_chunk<BUF>(a, rsrc, recs, start, len, 3) : make_uint4(0, 0, 0, 0);
                own[4] = nb > 64 ? own_chunk<BUF>(a, rsrc, recs, start, len, 4) : make_uint4(0, 0, 0, 0);
            }
        }
        st = tx_finish<kNS>(own, mine, 0u, len, false, present, fld, val);
    } else {
        // ---- unaligned region (rare): the whole wave sums one datagram at a time ----
        wave_serial_sums<NT, BUF>(a, rsrc, lane, __ballot(present), start, len, mine);
        // each owner takes chunks 0-5 from the 16-byte boundary below its start (its first
        // 81-96 bytes)
        const uint64_t b0 = start & ~15ull;
        const uint32_t s0 = static_cast<uint32_t>(start & 15);
        uint4 own[6];
#pragma unroll
        for (int i = 0; i < 6; ++i)
            own[i] = own_chunk<BUF>(a, rsrc, recs, b0, present ? s0 + len : 0u, i);
        st = tx_finish<6>(own, mine, s0, len, start & 1, present, fld, val);
    }
    // (after the wave's loads: a store between a load and its use would join the in-order
    // vmcnt queue)
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (fld[k] != kNoField)
            store_field<BUF, RNS_ROWS_TX_FIELD_AUX>(a, rsrc, start + fld[k], val[k]);
    if (live && a.status)
        a.status[p] = st;
}

}  // namespace rns
