// Receive verify through the rows: the packed form (csum_rows_rx_kernel) and datagrams at a fixed
// stride (csum_strided_rx_kernel).
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_rows.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// Receive verify through the rows decomposition (rns_rx_verify_packed_dev, round 5):
// ip_input_v4 (ip.rs:65-92), ip_input_v6 (ip.rs:114-121), tcp::validate_checksum
// (tcp.rs:838-850), icmp_input_v4/v6 (icmp.rs:44-75) over a packed arena of datagrams.  The
// whole datagram's word sum T comes from csum_rows_kernel's rows (P(e-1) - P(c0-1) + the
// owner's end chunk: no LDS table, no fences); each owner also loads its datagram's first 4
// chunks (64 bytes: every IPv4 header incl. options, the IPv6 header) a group of rows ahead
// of the row that streams them, as it loads its end chunk, and finishes exactly as the class
// kernel's receive verify does (rx_finish: header sum H, pseudo-header from the header's own
// addresses, L4 = T - H).  A unit of ACK-sized datagrams (all <= 64 B) skips the rows: each
// owner loads its datagram whole; a unit that does not start 16-byte aligned takes the
// per-datagram wave loop.
// ---------------------------------------------------------------------------
#ifndef RNS_ROWS_RX_OCC  // waves/SIMD bound of the receive form (its header chunks need registers)
#define RNS_ROWS_RX_OCC 6  // (78 VGPRs, no scratch; 5 with all 4 header chunks loaded with the rows)
#endif
// (Arenas of ACK-sized datagrams — at most 128 arena bytes per datagram — go to csum_stream_kernel,
// whose identical ACK path measured faster there: 64-byte datagrams 14.54-14.64 us per isolated
// dispatch against 15.03-15.25 for this kernel, at 6 or 8 waves/SIMD, with or without an LDS
// reservation like the stream kernel's; sessions r05g, r05h.)
template <bool NT, bool BUF, int D>
__global__ __launch_bounds__(64, RNS_ROWS_RX_OCC) void csum_rows_rx_kernel(const CsumArgs a)
{
    constexpr int kNS = 4;  // header chunks per datagram (16-byte-aligned: its first 64 bytes)
    const uint32_t lane = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.arena), static_cast<short>(0), static_cast<int>(BUF ? buf_records(a) : 0), 0x00020000);
    const uint64_t recs = buf_records(a);
    const PackedUnit u = packed_unit(a, lane);
    const uint64_t p = u.p, r0 = u.r0, start = u.start();
    const uint32_t len = u.len, excl = u.excl, total = u.total;
    const bool live = u.live, ok = u.ok(a);
    uint32_t mine = 0;
    uint4 own[kNS + 1];
    own[kNS] = make_uint4(0, 0, 0, 0);
    // the owner's finish (rx_finish), called in each path with that path's start offset and
    // parity: constants on the aligned paths, so their finish keeps only the aligned code
    auto finish = [&](uint32_t s0, bool odd) {
        uint32_t l4_res = 0;
        const uint8_t stv = rx_finish<kNS + 1>(a, own, mine, s0, len, odd, false, live && ok && len != 0, l4_res);
        if (live)
            store_rx_status(a, p, stv, l4_res);
    };
    if ((r0 & 15) == 0 && !__ballot(len > 64)) {
        // ---- ACK-sized unit: every owner takes its datagram whole ----
        mine = ack_unit_sum<BUF, true>(a, rsrc, recs, start, len, own);  // (rx_finish sees zeros past the end)
        finish(0u, false);
    } else if ((r0 & 15) == 0) {
        // ---- the rows: T, and the owner's first chunks loaded a group ahead ----
        const uint32_t c0 = excl >> 4;
        const uint32_t e = len ? (excl + len - 1) >> 4 : c0;
        // (3 header chunks with the rows, the 4th only where needed: 78 VGPRs, 6 waves/SIMD — IMIX
        // 448.0-448.4 -> 444.8-445.0 us, c3 isolated 234.1-234.3 -> 232.6-232.7 against all 4 at 5
        // waves/SIMD, session r05j)
        mine = rows_region_sum<NT, BUF, D, 3>(a, rsrc, recs, r0, total, c0, e, len, own);
        {
            // bytes 48..63 belong to the header only of an IPv4 datagram with more than 28 bytes of
            // options (IHL > 12); the IPv6 header is 40 bytes: those few owners load chunk 3 now
            const uint32_t b0 = own[0].x & 0xffu;
            const bool need = live && len > 48 && (b0 >> 4) == 4 && (b0 & 15u) > 12;
            if (__ballot(need))
                own[3] = need ? own_chunk<BUF>(a, rsrc, recs, start, len, 3) : make_uint4(0, 0, 0, 0);
            else
                own[3] = make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < kNS; ++i)  // zeros past the datagram's end (the region's next bytes)
            if (16u * i + 16u > len)
                own[i] = 16u * i < len ? keep_first(own[i], len - 16u * i) : make_uint4(0, 0, 0, 0);
        finish(0u, false);
    } else {
        // ---- unaligned region (rare): the whole wave sums one datagram at a time ----
        wave_serial_sums<NT, BUF>(a, rsrc, lane, __ballot(len != 0 && ok), start, len, mine);
        // each owner takes its header from the 16-byte boundary below its start: 5 chunks hold
        // its first 65-80 bytes, masked to the datagram
        const uint32_t s0 = unaligned_head<BUF>(a, rsrc, recs, start, len, len && ok, own);
        finish(s0, r0 & 1);  // every datagram of the range shares the region start's misalignment
    }
}

// ---------------------------------------------------------------------------
// Receive verify of datagrams at a fixed stride (rns_rx_verify_strided_dev, round 6):
// datagram i = arena[first_off + i * stride, + len16[i]) — a receive ring of fixed-size slots
// (64-byte ACK slots, or the reference's 2048-byte MRU buffers, netif.rs:66).  No block offsets
// and no scan: the lanes compute every address themselves.  With 16-byte-aligned slots a
// 64-datagram batch is read as csum_strided_tiny_kernel reads c2 — 4 rows, lane 4k + j loading
// chunk j of datagram 16r + k in row r (one coalesced KiB per row for 64-byte slots) — and
// lane 4k + j OWNS datagram 16j + k, so everything a datagram's finish needs stays in its quad:
// per row the quad sums its datagram's first 64 bytes (T) and its header bytes (H, IHL from
// byte 0 broadcast in the quad), and the owner (quad lane r) takes T, H and the first 24 bytes
// with quad DPP moves — no LDS, no ds_bpermute.  (Lane-per-datagram loads, as the packed
// form's ACK path does, measured 15.1-15.6 us per isolated dispatch on 1M x 64 B: r06b.)  A
// datagram longer than 64 bytes has its whole sum taken by the wave, one datagram at a time
// (as the packed kernels' unaligned path); its header is in the quad's 64 bytes.  Unaligned
// slots take that loop for every datagram and load their header chunks from the 16-byte
// boundary below the start.  B 64-datagram batches per wave.
// ---------------------------------------------------------------------------
constexpr int kStridedRxB = 1;    // 64-datagram batches per wave (k_packed.hip: launch_strided_rx)
constexpr int kStridedRxOcc = 8;  // waves/SIMD bound (48 VGPRs: 10 fit)
template <bool BUF, int B>
__global__ __launch_bounds__(64, kStridedRxOcc) void csum_strided_rx_kernel(const CsumArgs a)
{
    const uint32_t lane = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.arena), static_cast<short>(0), static_cast<int>(BUF ? buf_records(a) : 0), 0x00020000);
    const uint64_t recs = buf_records(a);
    const uint64_t start0 = a.first_off + a.base_adjust;
    const bool aligned = ((start0 | a.stride) & 15) == 0;  // uniform: kernel arguments
    const uint32_t k = lane >> 2, j = lane & 3;
    const uint32_t dl = 16u * j + k;  // the datagram this lane owns, in its batch
    uint32_t len[B];
    uint4 x[B][4];  // row r: chunk j of datagram 16r + k
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const uint64_t base = (static_cast<uint64_t>(blockIdx.x) * B + b) * 64;
        const uint64_t p = base + dl;
        len[b] = p < a.n ? static_cast<uint32_t>(a.len16[p]) : 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t q = base + 16u * r + k;
            const uint64_t o = start0 + q * a.stride + 16u * j;
            x[b][r] = load16<BUF, true>(a, rsrc, o, aligned && q < a.n && o + 16 <= recs);
        }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const uint64_t p = (static_cast<uint64_t>(blockIdx.x) * B + b) * 64 + dl;
        const bool live = p < a.n;
        const uint32_t L = len[b];
        const uint64_t start = start0 + p * a.stride;
        const bool ok = start <= a.arena_bytes && L <= a.arena_bytes - start;
        const bool present = live && ok && L != 0;
        uint32_t mine = 0;
        uint8_t stv;
        uint32_t l4_res = 0;
        if (aligned) {
            uint32_t H = 0, head[6] = {0, 0, 0, 0, 0, 0};
            auto row = [&](auto rc) {
                constexpr int r = decltype(rc)::value;
                const uint32_t Lr = dpp_mov<r * 0x55>(L);  // the row's datagram 16r + k: owned by quad lane r
                uint4 xm = x[b][r];
                if (16u * j + 16u > Lr)  // bytes past the datagram never count
                    xm = 16u * j < Lr ? keep_first(xm, Lr - 16u * j) : make_uint4(0, 0, 0, 0);
                const uint32_t t = group_allreduce<4>(sad4(xm, 0u));
                const uint32_t c0x = dpp_mov<0x00>(xm.x), c0y = dpp_mov<0x00>(xm.y);  // chunk 0 (quad lane 0)
                const uint32_t c0z = dpp_mov<0x00>(xm.z), c0w = dpp_mov<0x00>(xm.w);
                const uint32_t c1x = dpp_mov<0x55>(xm.x), c1y = dpp_mov<0x55>(xm.y);  // chunk 1 (quad lane 1)
                if (j == static_cast<uint32_t>(r)) {
                    mine = t;
                    head[0] = c0x;
                    head[1] = c0y;
                    head[2] = c0z;
                    head[3] = c0w;
                    head[4] = c1x;
                    head[5] = c1y;
                }
            };
            row(std::integral_constant<int, 0>{});
            row(std::integral_constant<int, 1>{});
            row(std::integral_constant<int, 2>{});
            row(std::integral_constant<int, 3>{});
            // H, the header's word sum (IHL*4 bytes, or 40 for IPv6): from the owner's first 20
            // bytes when no datagram of the wave has a longer header (IPv4 without options, the
            // ACK case), else per row from the quad's chunks like T
            const uint32_t hb0 = head[0] & 0xffu, hv = hb0 >> 4;
            const uint32_t hdr = hv == 4 ? (hb0 & 15u) * 4u : hv == 6 ? 40u : 0u;  // <= 60
            if (!__ballot(present && hdr > 20u)) {
#pragma unroll
                for (uint32_t d = 0; d < 5; ++d)
                    H = __builtin_amdgcn_sad_u16(4u * d < hdr ? head[d] : 0u, 0, H);
            } else {
                auto hrow = [&](auto rc) {
                    constexpr int r = decltype(rc)::value;
                    const uint32_t hr = dpp_mov<r * 0x55>(hdr);  // the row's datagram's header length
                    const uint4 xv = x[b][r];
                    uint4 hm = make_uint4(0, 0, 0, 0);
                    if (16u * j < hr)
                        hm = 16u * j + 16u <= hr ? xv : keep_first(xv, hr - 16u * j);
                    const uint32_t h = group_allreduce<4>(sad4(hm, 0u));
                    H = j == static_cast<uint32_t>(r) ? h : H;
                };
                hrow(std::integral_constant<int, 0>{});
                hrow(std::integral_constant<int, 1>{});
                hrow(std::integral_constant<int, 2>{});
                hrow(std::integral_constant<int, 3>{});
            }
            // longer datagrams: the whole wave sums one at a time
            wave_serial_sums<true, BUF>(a, rsrc, lane, __ballot(present && L > 64), start, L, mine);
            // rx_finish with H and the header dwords from the quad (16-byte-aligned: even starts)
            const RxParse rp = present ? rx_parse(head, L, a.local4_sum, a.local6_sum) : RxParse{kMetaMalformed, 0u, 0u};
            uint32_t hdr_res = 0;
            if (!(rp.meta & kMetaMalformed)) {
                hdr_res = finalize_bits(H, false, false, 0u, true, RNS_FLAG_COMPLEMENT);
                if (rp.meta & kMetaL4Checked)
                    l4_res = finalize_bits(mine - H, false, false, rp.ph, true, RNS_FLAG_COMPLEMENT);
            }
            stv = rx_verdict(rp.meta, hdr_res, l4_res);
        } else {
            // ---- unaligned slots (rare): the whole wave sums one datagram at a time ----
            wave_serial_sums<true, BUF>(a, rsrc, lane, __ballot(present), start, L, mine);
            // the header from the 16-byte boundary below the start: 5 chunks hold its first
            // 65-80 bytes, masked to the datagram
            const uint64_t b0 = start & ~15ull;
            const uint32_t s0 = static_cast<uint32_t>(start & 15);
            uint4 hd[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                hd[i] = own_chunk<BUF>(a, rsrc, recs, b0, present ? s0 + L : 0u, i);
                const int lo = static_cast<int>(s0) - 16 * i, hi = static_cast<int>(s0 + L) - 16 * i;
                hd[i] = make_uint4(keep_bytes(hd[i].x, lo, hi, 0), keep_bytes(hd[i].y, lo, hi, 4),
                                   keep_bytes(hd[i].z, lo, hi, 8), keep_bytes(hd[i].w, lo, hi, 12));
            }
            stv = rx_finish<5>(a, hd, mine, s0, L, start & 1, false, present, l4_res);
        }
        if (live)  // lane 4k + j: datagram 16j + k (a permutation of 64 consecutive entries)
            store_rx_status(a, p, stv, l4_res);
    }
}

}  // namespace rns
