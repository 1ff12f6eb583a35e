// TCP segmentation offload (rns_tx_segment_dev): tcp_write's segment loop on the device.
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_pool_tx.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// tcp_write (tcp.rs:256-285) cuts one send into send_mss pieces and sends each through
// send_packet -> tcp_output -> ip_output with the same ports, ack, window, flags and addresses: the
// heads of one send differ in the sequence number (+ the piece length), the IPv4 id
// (NEXT_PACKET_ID.fetch_add(1)) and the two length fields only.  So one template head per send
// ("flow") plus (data offset, data length, mss) implies every datagram of the send, and nothing
// per datagram crosses the bus but the finished heads on their way back.
//
// A wave owns 64 consecutive segments, a lane one segment:
//   - its flow: d_blk_flow names the flow of the wave's first segment; from there the wave loads
//     64 entries of d_seg_first at a time and every lane counts the flows that end at or before
//     its segment (readlane, no memory traffic), until a chunk's last flow ends past the wave's
//     last segment — one chunk unless empty flows lie between (they are skipped by the count) —
//     and at most n_flows entries in all.  The lane then checks seg_first[f] <= s < seg_first[f+1]
//     itself, so a wrong d_blk_flow or a d_seg_first that is not ascending costs results
//     (RNS_TX_MALFORMED), never a read outside the arrays.
//   - the flow's checks read the flow's descriptors and its template only, so every segment of a
//     flow decides alike and a rejected flow's head range stays untouched.
//   - the head: the lane copies the template dword by dword into its LDS slot, patching the
//     length, id and sequence fields and zeroing the two checksum fields, and sums the big-endian
//     words of the IP header, of the addresses and of the TCP header as it goes — no second pass.
//   - the payload slice (any byte alignment; odd for an odd mss) goes through the chain kernels'
//     class pass, which sums LE words paired by address exactly at any start; one swap (none at
//     an odd start) gives the fragment's big-endian sum, which folds onto
//     fold(pseudo-header + TCP header) as util.rs:112-119 folds the second fragment of the chain
//     [(head), (payload)].  The TCP header has even length, so this is also
//     compute_buffer_ones_comp over the reference's own 512-byte fragments: every fragment it
//     folds but the last has even length, and then per-fragment folding equals one flat sum.
//   - the finished heads go from LDS to the arena.  The lanes' slots lie back to back in LDS (a DPP
//     scan of the head lengths), so when the wave's heads are one run in the arena too — every
//     live segment well formed and its head where the one before ends, as the layout helper lays
//     the flows' ranges, the run 4-byte aligned — the staged bytes ARE the run: whole 16-byte
//     chunks, coalesced, and up to three dwords at either edge (the per-lane dword stores this
//     replaces, 40 bytes 40 bytes apart, cost 44 us of 295 on 1M MTU segments).  In any other
//     wave a lane writes its own head: dwords at a 4-byte-aligned address, bytes otherwise.
//     Either way only bytes of well-formed flows' head ranges are written, and all of them.
// ---------------------------------------------------------------------------
#ifndef RNS_SEG_AB  // attribution builds only (make ab): 1 = the heads are built but not stored, 2 = no payload pass
#define RNS_SEG_AB 0
#endif
#ifndef RNS_SEG_RUN_AUX  // cache-policy bits of the run write-back's chunk stores
#define RNS_SEG_RUN_AUX kNtAux
#endif
constexpr uint32_t kSegHeadMax = 100;             // 40 (IPv6) + 60 (TCP, doff 15)
constexpr uint32_t kSegSlotDw = kSegHeadMax / 4;  // 25: an odd dword stride, no LDS bank conflicts

template <bool NT, bool BUF>
__global__ __launch_bounds__(64, (NT && BUF) ? 4 : 3) void tx_segment_kernel(const CsumArgs a)
{
    __shared__ uint32_t hd[64 * kSegSlotDw];  // the wave's heads back to back, in lane order
    const uint32_t lane = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.arena), static_cast<short>(0), static_cast<int>(BUF ? buf_records(a) : 0), 0x00020000);
    const uint32_t blk = blockIdx.x, base = blk * 64u;  // one wave per 64 segments (launch_tx_segment)
    if (base >= a.n)
        return;
    const uint32_t s = base + lane;  // (the host caps a.n at RNS_CHAIN_MAX_PACKETS: no wrap)
    const bool live = s < a.n;
    const uint32_t last = min(base + 63u, a.n - 1u);

    // the lane's flow
    const uint32_t f0 = min(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(a.blk_flow[blk]))), a.n_flows);
    uint32_t cnt = 0;
    for (uint64_t g = f0; g < a.n_flows; g += 64) {
        const uint64_t idx = g + 1 + lane;  // the end of flow g + lane
        const uint32_t e = idx <= a.n_flows ? a.first[idx] : 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < 64; ++k)
            cnt += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(e), k)) <= s ? 1u : 0u;
        if (static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(e), 63)) > last)
            break;
    }
    const uint64_t f = static_cast<uint64_t>(f0) + cnt;
    bool ok = live && f < a.n_flows;

    // the flow's descriptors and checks
    uint32_t hl = 0, pl = 0, mss = 0, sf0 = 0, sf1 = 0, iphdr = 0;
    uint64_t po = 0, ho = 0;
    bool v4 = false;
    const uint8_t *t = a.tmpl;
    if (ok) {
        sf0 = a.first[f];
        sf1 = a.first[f + 1];
        hl = a.head_len8[f];
        pl = a.len[f];
        mss = a.len16[f];
        po = a.seg_pay_off[f];
        ho = a.seg_head_off[f];
        t += f * a.tmpl_stride;
        ok = sf0 <= s && s < sf1 && sf1 <= a.n && hl >= 40u && hl <= kSegHeadMax && hl <= a.tmpl_stride && mss >= 1u &&
             hl + mss <= 65535u;
    }
    if (ok) {
        const uint32_t b0 = t[0];
        v4 = b0 == 0x45u;
        iphdr = v4 ? 20u : 40u;
        ok = (v4 || (b0 >> 4) == 6u) && hl >= iphdr + 20u;
    }
    if (ok) {
        const uint32_t proto = v4 ? t[9] : t[6], doff = t[iphdr + 12u] >> 4;
        const uint32_t nseg = pl / mss + (pl % mss ? 1u : 0u);
        const uint64_t room = a.arena_bytes - a.base_adjust;  // the caller's arena_bytes
        ok = proto == 6u && doff >= 5u && iphdr + 4u * doff == hl && sf1 - sf0 == nseg && po <= room && pl <= room - po &&
             ho <= room && static_cast<uint64_t>(nseg) * hl <= room - ho;
    }
    const uint32_t j = s - sf0;
    const uint64_t skip = static_cast<uint64_t>(j) * mss;  // < pl: j < nseg
    const uint32_t seglen = ok ? static_cast<uint32_t>(min(static_cast<uint64_t>(mss), pl - skip)) : 0u;

    // the head, from the template into the lane's slot (the slots back to back: a DPP scan of the lengths)
    const uint32_t nd = ok ? hl >> 2 : 0u, ipd = iphdr >> 2, tcplen = hl - iphdr + seglen;
    const uint32_t posd = wave_excl_scan(nd);
    const uint32_t T = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(posd + nd), 63));  // <= 64 * 25
    uint32_t *slot = hd + posd;
    [[maybe_unused]] uint32_t keep = 0;
    TcpHeadSum hs;
    for (uint32_t k = 0; k < nd; ++k) {
        uint32_t d;
        __builtin_memcpy(&d, t + 4u * k, 4);
        if (v4) {
            if (k == 0)  // ip.rs:146: total length
                d = (d & 0xffffu) | (bswap16_u32(hl + seglen) << 16);
            if (k == 1)  // ip.rs:147: id
                d = (d & 0xffff0000u) | bswap16_u32((bswap16_u32(d & 0xffffu) + j) & 0xffffu);
            if (k == 2)  // the header checksum as zero
                d &= 0xffffu;
        } else if (k == 1) {  // ip.rs:168: payload length
            d = (d & 0xffff0000u) | bswap16_u32(tcplen & 0xffffu);
        }
        if (k == ipd + 1u)  // tcp.rs:945: seq
            d = __builtin_bswap32(__builtin_bswap32(d) + static_cast<uint32_t>(skip));
        if (k == ipd + 4u)  // the TCP checksum as zero
            d &= 0xffff0000u;
        slot[k] = d;
        hs.add(k, d, v4, ipd);
    }
    const uint32_t ipv = hs.ip_csum(), acc1 = hs.l4_head(tcplen);

    // the payload slice
    uint64_t d_start = ok ? po + a.base_adjust + skip : 0u;
    uint32_t pos;
    const uint32_t w = wave_class_pass<NT, BUF, kStashNone, kChainTiny && !NT>(a, rsrc, d_start, (RNS_SEG_AB & 2) ? 0u : seglen,
                                                                               0u, lane, nullptr, pos);
    const uint32_t x = fold16(w);
    const uint32_t t2 = acc1 + ((d_start & 1) ? x : bswap16_u32(x));
    const uint32_t r = ((t2 & 0xffffu) + (t2 >> 16)) ^ 0xffffu;

    if (ok) {
        if (v4)
            slot[2] |= bswap16_u32(ipv) << 16;
        slot[ipd + 4u] |= bswap16_u32(r);
    }
    const uint64_t dst = ok ? ho + a.base_adjust + static_cast<uint64_t>(j) * hl : 0u;
    wave_lds_fence();  // the write-back reads other lanes' heads
    // The wave's heads as one run: every live segment well formed, its head where the one before ends
    // (the flows' head ranges back to back, as rns_tx_segment_layout lays them), the run 4-byte aligned.
    // Then the staged heads are one contiguous region of the arena and go out as whole 16-byte chunks,
    // coalesced, with up to three dwords at either edge; any other wave's lanes write their own heads.
    const uint64_t D0 = first_lane_u64(dst);
    const bool in_run = !live || (ok && dst == D0 + 4ull * posd);
    const bool one_run = !__ballot(!in_run) && (D0 & 3) == 0;
    if (RNS_SEG_AB & 1) {
        keep = ok ? slot[2] ^ slot[ipd + 4u] : 0u;  // keeps the head build alive
    } else if (one_run) {
        uint8_t *w8 = const_cast<uint8_t *>(a.arena) + D0;
        const uint32_t lead = min(T, static_cast<uint32_t>((16u - (static_cast<uint32_t>(D0) & 15u)) & 15u) >> 2);
        const uint32_t nfull = (T - lead) >> 2, tail0 = lead + 4u * nfull;
        if (lane < lead)
            reinterpret_cast<uint32_t *>(w8)[lane] = hd[lane];
        for (uint32_t c = lane; c < nfull; c += 64) {
            const uint32_t q = lead + 4u * c;
            if constexpr (BUF) {  // nontemporal chunk stores, as the chain finalize's run write-back (RNS_TXFIN_RUN_AUX)
                const u32x4 y = {hd[q], hd[q + 1u], hd[q + 2u], hd[q + 3u]};
                __builtin_amdgcn_raw_buffer_store_b128(y, rsrc, static_cast<uint32_t>(D0 + 4ull * q), 0, RNS_SEG_RUN_AUX);
            } else {
                *reinterpret_cast<uint4 *>(w8 + 4ull * q) = make_uint4(hd[q], hd[q + 1u], hd[q + 2u], hd[q + 3u]);
            }
        }
        if (lane < T - tail0)
            reinterpret_cast<uint32_t *>(w8)[tail0 + lane] = hd[tail0 + lane];
    } else if (ok) {
        uint8_t *w8 = const_cast<uint8_t *>(a.arena) + dst;
        if ((dst & 3) == 0) {
            for (uint32_t k = 0; k < nd; ++k)
                reinterpret_cast<uint32_t *>(w8)[k] = slot[k];
        } else {
            for (uint32_t k = 0; k < nd; ++k) {
                const uint32_t d = slot[k];
                w8[4u * k] = static_cast<uint8_t>(d);
                w8[4u * k + 1u] = static_cast<uint8_t>(d >> 8);
                w8[4u * k + 2u] = static_cast<uint8_t>(d >> 16);
                w8[4u * k + 3u] = static_cast<uint8_t>(d >> 24);
            }
        }
    }
    if (live && a.status)  // 64 consecutive bytes per wave
        a.status[s] = ok ? static_cast<uint8_t>(((v4 ? RNS_TX_IP_FILLED : 0u) | RNS_TX_L4_FILLED) ^ (keep & 0x40u))
                         : static_cast<uint8_t>(RNS_TX_MALFORMED);
}

}  // namespace rns
