// Receive verify over fragment chains (rns_rx_verify_chain_dev): the chain kernel's receive form.
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_chain.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// A received datagram as the reference holds it: a NetBuffer chain (recv_packet,
// netif.rs:65-83: new_prealloc(2048) = four 512-byte pool fragments, trim_tail).
// ip_input (ip.rs:38-131) parses header() — the FIRST fragment only — trims the IP
// header (trim_head, buf.rs:294-329) and the transport input folds the rest fragment
// by fragment (compute_buffer_ones_comp, util.rs:112-119).
//
// A wave owns K*64 datagrams, as in csum_chain_kernel; their fragments stream through
// the class pass 64 at a time, in its kStashHead mode: the lanes that load a fragment's
// first five chunks also copy them to LDS (the flat receive verify's stash, one slot per
// fragment of the pass), so a head fragment's bytes are read once.  In the pass that
// holds its head fragment, the owner lane parses header() from that fragment's slot
// (rx_parse<true>: the first fragment's length len0 in place of the flat length) and
// sums the header's LE words H.  hdr (IHL*4 or 40) is even, so the trimmed head fragment
// pairs its words exactly as the whole fragment does: its contribution is
// fold(W_head - H), W_head the head fragment's raw sum from the class pass (the
// subtraction of rx_finish and of the chain kernel's FILL mode).  H alone gives the IPv4
// header verdict.  The pseudo-header needs the L4 length T - hdr, T = the sum of the
// fragment lengths: T is accumulated in the owner loop and the seed (partial: addresses +
// protocol, from the parse) is completed and applied at the end — the same residue mod
// 0xffff, zero iff everything is zero, while no fragment wraps the u32 accumulator.
//
// Two shapes break this and take the exact per-datagram loop at the end (rx_chain_slow,
// the whole wave on one datagram at a time): an IPv6 header that runs past its first
// fragment (24 <= len0 < 40: trim_head removes whole fragments and advances the next
// one's start, possibly to an odd byte), and a datagram with a fragment past 128 KiB
// (the seed enters the wrapping u32 accumulator, util.rs:89-99, so it cannot be applied
// afterwards).  An empty fragment after the first adds nothing (the reference panics on
// it, util.rs:92: parity unpinned).
//
// Per-datagram state in LDS across the class pass: [0] f0, [1] f1, [2] the running sum
// (low 16) and the kRx* flags, [3] the parse (meta | header verdict | hdr | partial
// seed; malformed until the head fragment has been seen), [4] H, [5] T.
// ---------------------------------------------------------------------------
constexpr uint32_t kRxBad = 0x80000000u;   // a fragment outside the arena / a malformed range: MALFORMED
constexpr uint32_t kRxSlow = 0x40000000u;  // the exact per-datagram loop decides the L4 sum
constexpr uint32_t kRxOvf = 0x20000000u;   // T passed 2^32 (overlapping fragments only): T >= 40 holds
constexpr uint32_t kRxHdrOk = 0x80u;       // pk[3]: compute_checksum(header[..hdr]) == 0
constexpr int kRxPk = 6;

constexpr int kRxNS = kStashChunks<kStashHead>;  // chunks stashed per fragment: its first 65+ bytes at any start

// The class pass over one batch of 64 fragments (lane l: fragment [d_start, d_start + d_len),
// d_len 0 = nothing to read): the lane's fragment's word sum, as in csum_chain_kernel — arenas
// of 4 GiB or more load through a windowed buffer descriptor when the 64 fragments lie within one
// window below the buffer range, else with 64-bit addresses.  st: the pass's stash (kRxNS chunks
// per fragment), pos: the lane's fragment's slot in it.  (The window choice restates the one inside
// csum_chain_kernel, which is left as it is so that its instantiations keep their instructions.)
template <bool NT, bool BUF>
__device__ __forceinline__ uint32_t chain_pass_sum(const CsumArgs &a, __amdgpu_buffer_rsrc_t rsrc, uint64_t d_start,
                                                   uint32_t d_len, uint32_t lane, uint4 *st, uint32_t &pos)
{
    if constexpr (!BUF) {
        const uint32_t lo_hi = d_len ? static_cast<uint32_t>(d_start >> 32) : 0xFFFFFFFFu;
        const uint32_t wlh = wave_min_u32(lo_hi);
        const uint32_t wll = wave_min_u32(d_len && lo_hi == wlh ? static_cast<uint32_t>(d_start) & ~15u : 0xFFFFFFFFu);
        const uint64_t end = d_len ? d_start + d_len : 0;
        const uint32_t ehi = wave_max_u32(static_cast<uint32_t>(end >> 32));
        const uint32_t elo = wave_max_u32(static_cast<uint32_t>(end >> 32) == ehi ? static_cast<uint32_t>(end) : 0u);
        const uint64_t wlo = (static_cast<uint64_t>(wlh) << 32) | wll, whi = (static_cast<uint64_t>(ehi) << 32) | elo;
        if (whi <= wlo || whi - wlo <= kOobOffset - 4096u) {  // (no fragment: whi = 0)
            const uint64_t wb = whi > wlo ? wlo : 0;
            const uint64_t recs_w = buf_records(a) - wb;
            const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t *>(a.arena) + wb, static_cast<short>(0),
                static_cast<int>(recs_w < kOobOffset ? recs_w : kOobOffset), 0x00020000);
            return wave_class_pass<NT, true, kStashHead, kChainTiny && !NT>(a, rw, d_len ? d_start - wb : 0, d_len, 0u, lane,
                                                                            st, pos);
        }
        return wave_class_pass<NT, false, kStashHead, kChainTiny && !NT>(a, rsrc, d_start, d_len, 0u, lane, st, pos);
    } else {
        return wave_class_pass<NT, BUF, kStashHead, kChainTiny && !NT>(a, rsrc, d_start, d_len, 0u, lane, st, pos);
    }
}

// Owner lane, in the pass that holds its head fragment: own = that fragment's stash slot (its
// chunks 0..kRxNS-1 from the 16-byte-aligned chunk holding its first byte; a chunk past the
// fragment's end is stale and never read), s = start & 15, hl = its length (0: empty, or outside
// the arena).  Parses header() and sums the header's LE words (paired by address, as the class
// pass pairs the fragment's).  info = the parse packed for pk[3]; hsum = H (0 when the datagram is
// malformed or takes the exact loop).  Returns whether the datagram takes the exact loop (an
// IPv6 header past its first fragment).
__device__ __forceinline__ bool rx_chain_head(const CsumArgs &a, const uint4 *own, uint32_t s, uint32_t hl, bool odd,
                                              uint32_t &info, uint32_t &hsum)
{
    uint4 ch[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        ch[i] = own[i];
    uint32_t head[6];  // header()[0..24) in datagram byte order (bytes past hl are never read by the parse)
    if (s == 0) {      // 16-byte-aligned fragment (every NetBuffer): the dwords as they are
        const uint32_t w6[6] = {ch[0].x, ch[0].y, ch[0].z, ch[0].w, ch[1].x, ch[1].y};
#pragma unroll
        for (int k = 0; k < 6; ++k)
            head[k] = w6[k];
    } else {
        head_from_stash(ch, s, head);
    }
    const RxParse rp = rx_parse<true>(head, hl, a.local4_sum, a.local6_sum);  // (hl == 0: header[0] panics)
    info = rp.meta | (rp.hdr << 8) | (rp.ph << 16);
    hsum = 0;
    if (rp.meta & kMetaMalformed)
        return false;
    if (rp.hdr > hl)  // IPv6, 24 <= len0 < 40
        return true;
    const int hlo = static_cast<int>(s), hhi = hlo + static_cast<int>(rp.hdr);  // <= 15 + 60, inside the fragment
    uint32_t H;
    if (hlo == 0 && hhi == 20) {  // aligned IPv4 header, no options: 5 dwords
        H = __builtin_amdgcn_sad_u16(ch[0].x, 0, 0u);
        H = __builtin_amdgcn_sad_u16(ch[0].y, 0, H);
        H = __builtin_amdgcn_sad_u16(ch[0].z, 0, H);
        H = __builtin_amdgcn_sad_u16(ch[0].w, 0, H);
        H = __builtin_amdgcn_sad_u16(ch[1].x, 0, H);
    } else {
        H = stash_sum_le(ch, hlo, hhi);
        if (hhi > 48) {  // IPv6 past offset 8, IPv4 with options: header bytes in chunks 3-4
            const uint4 tail[2] = {own[3], own[4]};
            H += stash_sum_le(tail, hlo - 48, hhi - 48);
        }
    }
    hsum = H;
    if ((rp.meta & kMetaV6) || finalize_bits(H, odd, false, 0u, true, RNS_FLAG_COMPLEMENT) == 0)
        info |= kRxHdrOk;
    return false;
}

// The seed with the L4 length in it (util.rs:180-207: length as u16 in the IPv4 layout, as u32
// in the IPv6 one); ph = the parse's partial seed, 0 = no pseudo-header (ICMPv4).
__device__ __forceinline__ uint32_t rx_chain_seed(uint32_t info, uint32_t l4len)
{
    const uint32_t ph = info >> 16;
    if (ph == 0)
        return 0u;
    return fold16(ph + ((info & kMetaV4) ? (l4len & 0xffffu) : (l4len >> 16) + (l4len & 0xffffu)));
}

// The exact per-datagram loop, the whole wave on datagram [f0, f1) (wave-uniform arguments; every
// fragment inside the arena): trim_head(hdr) as buf.rs:294-329 does it — whole fragments go
// while their length does not exceed what remains, then the next one's start advances — and
// util.rs:88-106 per remaining fragment, the BE words paired from the fragment's own (trimmed)
// start in the wrapping u32 accumulator that starts from the running sum.
__device__ __forceinline__ uint32_t rx_chain_slow(const CsumArgs &a, uint32_t f0, uint32_t f1, uint32_t hdr,
                                                  uint32_t seed, uint32_t lane)
{
    uint32_t rem = hdr, acc = seed;
    for (uint32_t t = f0; t < f1; ++t) {
        uint64_t o = a.off[t] + a.base_adjust;
        uint32_t len = a.len[t];
        if (len <= rem) {  // removed whole (an empty one adds nothing either way)
            rem -= len;
            continue;
        }
        o += rem;
        len -= rem;
        rem = 0;
        const uint8_t *p = a.arena + o;
        const uint32_t nw = len >> 1;
        uint32_t part = 0;
        for (uint32_t j = lane; j < nw; j += 64)
            part += (static_cast<uint32_t>(p[2ull * j]) << 8) | p[2ull * j + 1];
        if ((len & 1u) && lane == 0)
            part += static_cast<uint32_t>(p[len - 1]) << 8;  // util.rs:97-99
        acc += group_sum<64>(part);                          // util.rs:89-99, mod 2^32
        acc = fold16(acc);                                   // util.rs:101-103
    }
    return acc;
}

// Waves/SIMD: 4 (128 VGPRs) for the nontemporal buffer form with one datagram per lane (NetBuffer
// chains of MTU datagrams), 3 for the rest — the 64-bit addresses need the registers, and with more
// datagrams per lane the per-datagram LDS state bounds the waves of a CU first.  KMAX = 1, 2
// (IMIX in 512-byte buffers: 1.5 fragments per datagram) or kChainMaxK sizes that state.
template <bool NT, bool BUF, uint32_t KMAX>
constexpr int rx_chain_occ()
{
#ifdef RNS_CHAIN_OCC
    return RNS_CHAIN_OCC;
#else
    return (NT && BUF && KMAX == 1) ? 4 : 3;
#endif
}

template <bool NT, bool BUF, uint32_t KMAX>
__global__ __launch_bounds__(kChainBlock, (rx_chain_occ<NT, BUF, KMAX>())) void rx_chain_kernel(const CsumArgs a)
{
    __shared__ uint32_t pk[kRxPk][KMAX * 64];
    __shared__ uint32_t fl[64];  // the pass's fragment lengths (len0, T)
    __shared__ uint4 st[64 * kRxNS];  // the pass's stash: every fragment's first chunks, by sorted position
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x;  // one-wave workgroups (kChainBlock)
    static_assert(kChainBlock == 64, "one wave per workgroup");
    const uint32_t K = KMAX == 1 ? 1u : a.chain_k;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.arena), static_cast<short>(0), static_cast<int>(BUF ? buf_records(a) : 0), 0x00020000);
    const uint64_t per_wave = 64ull * K;
    const uint64_t first_pkt = static_cast<uint64_t>(wave) * per_wave, step = static_cast<uint64_t>(gridDim.x) * per_wave;
    if (first_pkt >= a.n)
        return;
    for (uint32_t base = static_cast<uint32_t>(first_pkt);;) {
        uint32_t lo_all = 0xFFFFFFFFu, hi_all = 0u;
        for (uint32_t q = 0; q < K; ++q) {
            const uint64_t p = base + q * 64 + lane;  // (32-bit add: the host caps a.n at 2^32 - 64 * kChainMaxK)
            const bool live = p < a.n;
            uint32_t f0 = live ? a.first[p] : 0u, f1 = live ? a.first[p + 1] : 0u;
            const bool ok = f0 <= f1 && f1 <= a.n_frags;
            if (!ok)
                f0 = f1 = 0;
            lo_all = f0 < f1 ? min(lo_all, f0) : lo_all;
            hi_all = f0 < f1 ? max(hi_all, f1) : hi_all;
            pk[0][q * 64 + lane] = f0;
            pk[1][q * 64 + lane] = f1;
            pk[2][q * 64 + lane] = f0 < f1 ? 0u : kRxBad;  // no fragments (or a malformed range): header() asserts
            pk[3][q * 64 + lane] = kMetaMalformed;         // until the head fragment is parsed
            pk[4][q * 64 + lane] = 0u;
            pk[5][q * 64 + lane] = 0u;
        }
        // the wave's fragments: the union of its datagrams' ranges (contiguous for a CSR list)
        const uint32_t F0 = wave_min_u32(lo_all), F1 = wave_max_u32(hi_all);
        const uint32_t passes = (F1 - F0 + 63) / 64;  // (F1 >= F0, equal if no fragments)
        for (uint32_t it = 0; it < passes; ++it) {
            const uint32_t fb = F0 + 64u * it;  // < F1 <= n_frags: 32 bits
            uint64_t d_start = 0;
            uint32_t d_len = 0;
            if (static_cast<uint64_t>(fb) + lane < F1) {
                d_start = a.off[static_cast<uint64_t>(fb) + lane];
                d_len = a.len[static_cast<uint64_t>(fb) + lane];
            }
            d_start += a.base_adjust;
            const bool d_ok = d_start <= a.arena_bytes && d_len <= a.arena_bytes - d_start;
            if (!d_ok || d_len == 0) {  // an empty fragment adds nothing (the reference panics on it)
                d_len = 0;
                d_start = 0;
            }
            const bool big = d_len > kNoWrapBytes, odd = d_start & 1;
            wave_lds_fence();  // the previous pass's owners are done with fl and the stash
            fl[lane] = d_len;
            uint32_t pos;
            const uint32_t w = chain_pass_sum<NT, BUF>(a, rsrc, d_start, d_len, lane, st, pos);
            // the fragment's folded BE sum (RFC 1071 §2(B), as finalize_bits), bit 16 = past 128 KiB
            // (its datagram takes the exact loop), 17 = outside the arena, 18 = odd start, 19-22 =
            // start & 15, 23-28 = its stash slot
            const uint32_t x = fold16(w);
            const uint32_t gp = (big ? 0u : odd ? x : (((x & 0xff) << 8) | (x >> 8))) | (big ? 0x10000u : 0u) |
                                (d_ok ? 0u : 0x20000u) | (odd ? 0x40000u : 0u) |
                                (static_cast<uint32_t>(d_start & 15) << 19) | (pos << 23);
            wave_lds_fence();  // fl and the stash were written by other lanes of this wave
            // owner lanes: each datagram's fragments inside [fb, fb + 64), in order
            for (uint32_t q = 0; q < K; ++q) {
                const uint32_t i = q * 64 + lane;
                const uint32_t f0 = pk[0][i];
                uint32_t t = max(f0, fb);
                const uint32_t hi = static_cast<uint32_t>(min(static_cast<uint64_t>(pk[1][i]), static_cast<uint64_t>(fb) + 64));
                if (!__ballot(t < hi))
                    continue;
                uint32_t acc = pk[2][i], T = pk[5][i];
                // the head fragment: header() parsed from its stash slot; trimmed, it contributes its raw
                // sum without the header's words, folded here
                const bool headin = f0 >= fb && f0 < hi;
                const int hsrc = headin ? static_cast<int>(f0 - fb) : 0;
                const uint32_t hraw = static_cast<uint32_t>(__shfl(static_cast<int>(w), hsrc, 64));
                const uint32_t hf = static_cast<uint32_t>(__shfl(static_cast<int>(gp), hsrc, 64));
                uint32_t hsum = 0;
                if (headin) {
                    uint32_t info;
                    if (rx_chain_head(a, st + ((hf >> 23) & 63u) * kRxNS, (hf >> 19) & 15u, fl[hsrc], hf & 0x40000u, info, hsum))
                        acc |= kRxSlow;
                    pk[3][i] = info;
                    pk[4][i] = hsum;
                }
                const uint32_t hx = fold16(hraw - hsum);
                const uint32_t hg = (hf & 0x40000u) ? hx : (((hx & 0xff) << 8) | (hx >> 8));
                do {
                    const bool act = t < hi;
                    const int src = act ? static_cast<int>(t - fb) : 0;
                    const uint32_t gv = static_cast<uint32_t>(__shfl(static_cast<int>(gp), src, 64));
                    if (act) {
                        uint32_t s = (acc & 0xffffu) + (t == f0 ? hg : gv & 0xffffu);  // <= 0x1fffe
                        s = (s & 0xffff) + (s >> 16);                                   // one end-around step folds it
                        const uint32_t nt = T + fl[src];
                        acc = s | (acc & 0xffff0000u) | ((gv & 0x10000u) ? kRxSlow : 0u) | ((gv & 0x20000u) ? kRxBad : 0u) |
                              (nt < T ? kRxOvf : 0u);
                        T = nt;
                        ++t;
                    }
                } while (__ballot(t < hi));
                pk[2][i] = acc;
                pk[5][i] = T;
            }
        }
        wave_lds_fence();
        for (uint32_t q = 0; q < K; ++q) {
            const uint64_t p = base + q * 64 + lane;
            const uint32_t i = q * 64 + lane;
            const uint32_t acc = pk[2][i], T = pk[5][i];
            uint32_t info = pk[3][i];
            const uint32_t hdr = (info >> 8) & 0x3fu;
            if ((acc & kRxBad) || ((info & kMetaV6) && T < 40u && !(acc & kRxOvf)))  // (trim_head(40) asserts)
                info = kMetaMalformed;
            const bool checked = !(info & kMetaMalformed) && (info & kMetaL4Checked);
            const uint32_t seed = rx_chain_seed(info, T - hdr);
            uint32_t s = fold16((acc & 0xffffu) + seed);
            // the exact loop, one datagram at a time
            for (uint64_t m = __ballot(p < a.n && checked && (acc & kRxSlow)); m; m &= m - 1) {
                const int l = static_cast<int>(__builtin_ctzll(m));
                const uint32_t r = rx_chain_slow(a, static_cast<uint32_t>(__shfl(static_cast<int>(pk[0][i]), l, 64)),
                                                 static_cast<uint32_t>(__shfl(static_cast<int>(pk[1][i]), l, 64)),
                                                 static_cast<uint32_t>(__shfl(static_cast<int>(hdr), l, 64)),
                                                 static_cast<uint32_t>(__shfl(static_cast<int>(seed), l, 64)), lane);
                s = static_cast<int>(lane) == l ? r : s;
            }
            const uint32_t l4_res = checked ? s ^ 0xffffu : 0u;
            const uint8_t stv = rx_verdict(info, (info & kRxHdrOk) ? 0u : 1u, l4_res);
            if (p < a.n) {
                a.status[p] = stv;  // 64 consecutive bytes per wave
                if (a.l4_out)
                    a.l4_out[p] = static_cast<uint16_t>(l4_res);  // 64 consecutive u16: one 128-byte store
            }
        }
        wave_lds_fence();  // the next batch rewrites pk
        const uint64_t next = static_cast<uint64_t>(base) + step;
        if (next >= a.n)
            break;
        base = static_cast<uint32_t>(next);
    }
}

}  // namespace rns
