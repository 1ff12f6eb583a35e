// Receive verify of datagrams held in fixed-size pool buffers (rns_rx_verify_pool_dev): the
// receive chain kernel's form for recv_packet's own layout, over compact descriptors.
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_chain_rx.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// recv_packet (netif.rs:65-83) reads a datagram into new_prealloc(2048), four 512-byte pool
// buffers (buf.rs:50), then trim_tail: a chain of FULL buffers and a last one that holds the
// remainder.  With buffers of B = 2^buf_log2 bytes at pool offsets idx * B, the chain of a
// datagram of T bytes is implied by T and the indices of its nf = ceil(T / B) buffers, so the
// descriptors are a u16 length per datagram, a u32 index per buffer and one u32 per 64 datagrams
// (CsumArgs: len16, off32 = the indices, first = d_blk_first, align_mask = B - 1).
//
// A wave owns K*64 datagrams.  Per 64-datagram block q each lane takes its length, nf, and the
// DPP prefix sum of nf: first_i = d_blk_first[block] + the sum before i.  The blocks' fragment
// ranges are independent of each other (each has its own d_blk_first entry), so the wave walks
// them concatenated: virtual fragment v of the wave = fragment v - V_q of block q, V_q the
// fragments of the blocks before q.  That bounds the passes by the lengths alone (K*64 datagrams
// of at most 2^16 / B buffers), whatever d_blk_first holds.  64 virtual fragments per pass: one
// coalesced 4-byte index load; every fragment is B bytes long except a datagram's last, whose
// owner writes the remainder into the pass's length row.  The bytes stream through the receive
// chain kernel's class pass (chain_pass_sum: kStashHead, the per-pass window past 4 GiB).
//
// What the chain kernel carries and this one does not, and why (6 <= buf_log2 <= 15, pool 16-byte
// aligned, both checked by the entry point):
//   - no unaligned head: every buffer starts at a multiple of B >= 64 from a 16-byte-aligned base,
//     so the head's dwords are the stashed ones (rx_chain_head with s = 0: head_from_stash and the
//     masked header sums at a byte shift fold away);
//   - no fragment past 128 KiB (B <= 32 KiB): the exact big-endian sum never runs;
//   - no odd start and no odd-length fragment before the last: every fragment's LE words are the
//     flat datagram's, so the owner adds the fragments' folded LE sums — a range of the pass's
//     prefix sum, not a loop over its fragments — and swaps the bytes once at the end (RFC 1071
//     §2(B));
//   - no header past the first buffer: an IPv4 header is at most 60 bytes and len0 = min(T, B)
//     with B >= 64, so hdr > len0 means hdr > T: malformed, as the parse says.  IPv6: len0 < 40
//     means T = len0 < 40, which trim_head(40) rejects: malformed.  So there is no kRxSlow state
//     and no exact per-datagram loop (rx_chain_slow).
//   - T is the datagram's length itself: nothing to accumulate, nothing to overflow.
//
// Per-datagram state in LDS: [0] its first virtual fragment, [1] its length (0: owns no fragment
// — empty, or its range runs past n_frags), [2] the running LE sum (low 16) | kRxBad, [3] the
// parse (as the chain kernel's pk[3]).
// ---------------------------------------------------------------------------
constexpr int kPoolPk = 4;
constexpr uint32_t kPoolMinLog2 = 6, kPoolMaxLog2 = 15;
static_assert((1u << kPoolMinLog2) >= 60u + 4u, "an IP header (<= 60 bytes) lies inside the first buffer");
static_assert((1u << kPoolMinLog2) % 16u == 0, "every buffer of a 16-byte-aligned pool starts 16-byte aligned");
static_assert((1u << kPoolMaxLog2) <= kNoWrapBytes, "no fragment takes the exact sum past 128 KiB");
static_assert(kRxNS * 16 >= 60, "the stash holds a whole IP header");
// the pass's prefix sum: 64 folded sums in bits 0-23, the count of fragments outside the pool above
static_assert(64u * 0xffffu < (1u << 24), "64 folded fragment sums fit below the rejected count");
constexpr uint32_t kPoolFragBad = 1u << 24;  // gp: the fragment lies outside the pool
constexpr int kPoolPosShift = 25;            // gp: the fragment's stash slot (6 bits)

template <bool NT, bool BUF, uint32_t KMAX>
__global__ __launch_bounds__(kChainBlock, (rx_chain_occ<NT, BUF, KMAX>())) void rx_pool_kernel(const CsumArgs a)
{
    __shared__ uint32_t pk[kPoolPk][KMAX * 64];
    __shared__ uint32_t fl[64];          // the pass's fragment lengths
    __shared__ uint32_t vq[KMAX + 1];    // V_q: the wave's virtual fragments before block q
    __shared__ uint32_t bq[KMAX];        // d_blk_first of block q
    __shared__ uint4 st[64 * kRxNS];     // the pass's stash: every fragment's first chunks, by sorted position
    const uint32_t lane = threadIdx.x & 63;
    static_assert(kChainBlock == 64, "one wave per workgroup");
    const uint32_t K = KMAX == 1 ? 1u : a.chain_k;
    const uint32_t bmask = a.align_mask, blog = static_cast<uint32_t>(__popc(bmask)), bbytes = bmask + 1u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.arena), static_cast<short>(0), static_cast<int>(BUF ? buf_records(a) : 0), 0x00020000);
    const uint64_t first_pkt = static_cast<uint64_t>(blockIdx.x) * 64ull * K;  // one batch per wave (launch_rx_pool)
    if (first_pkt >= a.n)
        return;
    const uint32_t base = static_cast<uint32_t>(first_pkt);
    uint32_t V = 0;
    for (uint32_t q = 0; q < K; ++q) {
        const uint64_t p = base + q * 64 + lane;  // (32-bit add: the host caps a.n at 2^32 - 64 * kChainMaxK)
        const uint32_t len = p < a.n ? a.len16[p] : 0u;
        const uint32_t nf = (len + bmask) >> blog;
        const uint32_t inc = wave_incl_scan(nf);  // <= 64 * 2^10
        const uint32_t blk = (base >> 6) + q;     // wave-uniform
        const uint32_t B = static_cast<uint64_t>(blk) * 64 < a.n ? a.first[blk] : 0u;
        // first_i + nf_i <= n_frags, in 64 bits: d_blk_first is the caller's
        const bool ok = nf != 0 && static_cast<uint64_t>(B) + inc <= a.n_frags;
        pk[0][q * 64 + lane] = V + (inc - nf);
        pk[1][q * 64 + lane] = ok ? len : 0u;
        pk[2][q * 64 + lane] = ok ? 0u : kRxBad;  // no fragments (header() asserts) or a range past n_frags
        pk[3][q * 64 + lane] = kMetaMalformed;    // until the head fragment is parsed
        if (lane == 0) {
            vq[q] = V;
            bq[q] = B;
        }
        V += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(inc), 63));
    }
    if (lane == 0)
        vq[K] = V;
    wave_lds_fence();
    const uint32_t passes = (V + 63) / 64;  // V <= 8 * 2^16
    for (uint32_t it = 0; it < passes; ++it) {
        const uint32_t fb = 64u * it, v = fb + lane;
        // the lane's fragment: its block, its place in d_buf_idx
        bool have = false;
        uint64_t gi = 0;
        for (uint32_t q = 0; q < K; ++q) {
            const uint32_t v0 = vq[q], v1 = vq[q + 1];
            if (v >= v0 && v < v1) {
                have = true;
                gi = static_cast<uint64_t>(bq[q]) + (v - v0);
            }
        }
        have = have && gi < a.n_frags;
        const uint32_t bi = have ? a.off32[gi] : 0u;  // 64 consecutive indices per block: one 256-byte load
        wave_lds_fence();  // the previous pass's owners are done with fl and the stash
        fl[lane] = bbytes;
        wave_lds_fence();
        for (uint32_t q = 0; q < K; ++q) {  // a datagram's last fragment holds the remainder
            const uint32_t i = q * 64 + lane;
            const uint32_t len = pk[1][i];
            const uint32_t last = pk[0][i] + ((len + bmask) >> blog) - 1u;
            if (len != 0 && last - fb < 64u)
                fl[last - fb] = len - ((len - 1u) & ~bmask);
        }
        wave_lds_fence();
        uint32_t d_len = have ? fl[lane] : 0u;
        uint64_t d_start = static_cast<uint64_t>(bi) << blog;
        const bool d_ok = d_start <= a.arena_bytes && d_len <= a.arena_bytes - d_start;
        if (!d_ok) {
            d_len = 0;
            d_start = 0;
        }
        uint32_t pos;
        const uint32_t w = chain_pass_sum<NT, BUF>(a, rsrc, d_start, d_len, lane, st, pos);
        // the fragment's folded LE sum, whether it lies outside the pool, its stash slot
        const uint32_t gp = fold16(w) | (d_ok ? 0u : kPoolFragBad) | (pos << kPoolPosShift);
        const uint32_t S = wave_incl_scan(gp & (2u * kPoolFragBad - 1u));
        wave_lds_fence();  // the stash was written by other lanes of this wave
        // owner lanes: each datagram's fragments inside [fb, fb + 64) are a lane range of this pass
        for (uint32_t q = 0; q < K; ++q) {
            const uint32_t i = q * 64 + lane;
            const uint32_t f0 = pk[0][i], len = pk[1][i];
            const uint32_t t = max(f0, fb), hi = min(f0 + ((len + bmask) >> blog), fb + 64u);
            const bool act = t < hi;
            if (!__ballot(act))
                continue;
            const int l_lo = act ? static_cast<int>(t - fb) : 0, l_hi = act ? static_cast<int>(hi - fb) - 1 : 0;
            const uint32_t s_hi = static_cast<uint32_t>(__shfl(static_cast<int>(S), l_hi, 64));
            const uint32_t s_lo = static_cast<uint32_t>(__shfl(static_cast<int>(S), max(l_lo, 1) - 1, 64));
            const uint32_t R = s_hi - (l_lo ? s_lo : 0u);
            uint32_t add = R & (kPoolFragBad - 1u);
            // the head fragment: header() parsed from its stash slot; trimmed, it contributes its raw
            // sum without the header's words
            const bool headin = act && f0 >= fb;
            if (__ballot(headin)) {
                const int hsrc = headin ? static_cast<int>(f0 - fb) : 0;
                const uint32_t hraw = static_cast<uint32_t>(__shfl(static_cast<int>(w), hsrc, 64));
                const uint32_t hf = static_cast<uint32_t>(__shfl(static_cast<int>(gp), hsrc, 64));
                if (headin) {
                    uint32_t info, hsum;
                    const uint32_t hl = (hf & kPoolFragBad) ? 0u : min(len, bbytes);
                    (void)rx_chain_head(a, st + ((hf >> kPoolPosShift) & 63u) * kRxNS, 0u, hl, false, info, hsum);
                    pk[3][i] = info;
                    add = add - (hf & 0xffffu) + fold16(hraw - hsum);
                }
            }
            if (act) {
                const uint32_t acc = pk[2][i];
                pk[2][i] = fold16((acc & 0xffffu) + add) | (acc & kRxBad) | (R >= kPoolFragBad ? kRxBad : 0u);
            }
        }
    }
    wave_lds_fence();
    for (uint32_t q = 0; q < K; ++q) {
        const uint64_t p = base + q * 64 + lane;
        const uint32_t i = q * 64 + lane;
        const uint32_t acc = pk[2][i], T = pk[1][i];
        uint32_t info = pk[3][i];
        const uint32_t hdr = (info >> 8) & 0x3fu;
        if ((acc & kRxBad) || ((info & kMetaV6) && T < 40u))  // (trim_head(40) asserts)
            info = kMetaMalformed;
        const bool checked = !(info & kMetaMalformed) && (info & kMetaL4Checked);
        const uint32_t le = acc & 0xffffu;
        const uint32_t s = fold16((((le & 0xffu) << 8) | (le >> 8)) + rx_chain_seed(info, T - hdr));
        const uint32_t l4_res = checked ? s ^ 0xffffu : 0u;
        const uint8_t stv = rx_verdict(info, (info & kRxHdrOk) ? 0u : 1u, l4_res);
        if (p < a.n) {
            a.status[p] = stv;  // 64 consecutive bytes per wave
            if (a.l4_out)
                a.l4_out[p] = static_cast<uint16_t>(l4_res);  // 64 consecutive u16: one 128-byte store
        }
    }
}

}  // namespace rns
