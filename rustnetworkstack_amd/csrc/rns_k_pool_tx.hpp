// Transmit finalize of datagrams held in fixed-size pool buffers (rns_tx_fill_pool_dev): the
// receive pool kernel's decomposition with the transmit finish, over compact descriptors.
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_pool_rx.hpp"
#include "rns_k_txrows.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// An outgoing datagram as the reference builds it: append_from_slice (buf.rs:385-420) fills whole
// pool buffers from offset 0 and a last one with the remainder, alloc_header (buf.rs:262-291)
// prepends a buffer whose data sits at its END and ip_output grows that downwards.  With buffers
// of B = 2^buf_log2 bytes at pool offsets idx * B, datagram i is implied by its head length, its
// payload length and the indices of its nf = 1 + ceil(pay / B) buffers: the head fragment is the
// last hl bytes of the first buffer, the others are read from their start (CsumArgs: head_len8,
// len16 = payload lengths, off32 = the indices, first = d_blk_first, align_mask = B - 1).
//
// The walk is rx_pool_kernel's: a wave owns K*64 datagrams, a DPP prefix sum of nf per 64-block
// gives every datagram its range of the wave's virtual fragments, and 64 virtual fragments per
// pass stream through the class pass with its stash of first chunks.  What differs:
//   - the head fragment starts at B - hl, at any byte alignment (odd for an odd hl).  The class
//     pass pairs its LE words by address, as it pairs every fragment's, so its raw sum W is
//     exact at any start; the owner parses it from its stash slot (tx_parse), takes the IP
//     header's words H (at most 15 + 60 bytes from the 16-byte boundary: always stashed) and the
//     L4 field's two bytes out of W, and folds the rest — the head's L4 part, a fragment of its
//     own, an odd length zero-padded by the edge mask — onto the pseudo-header: util.rs:112-119's
//     first step.  The IP header length is even, so that part pairs as the whole fragment does.
//     The field's bytes come from the stash too; only a field past the stash's 80 bytes (a TCP
//     field behind 44+ bytes of IPv4 options at an unlucky start) is read from memory, two bytes
//     by its owner alone.  So a head of any length up to 255 takes this one path: there is no
//     exact per-datagram loop.
//   - the payload fragments start 16-byte aligned and all but the last have even length: their
//     folded LE sums add as the flat payload's do (a range of the pass's prefix sum) and are
//     swapped once at the end, one more fragment fold after the head's.
//   - the owner stores the L4 field and the IPv4 header checksum into its head with the 2-byte
//     field store (store_field); heads are scattered, so there is no run to write back.
//
// Per-datagram state in LDS: [0] its first virtual fragment, [1] kPoolTxOwn | pay << 8 | hl (0: it
// owns no fragment — its range runs past n_frags), [2] the payload's running LE sum (low 16) |
// the head's fold (seed + head L4 part, high 16), [3] RNS_TX_* | the L4 field's offset << 8 | the
// IPv4 header checksum << 16 (RNS_TX_MALFORMED until the head is parsed, and again once a
// fragment outside the pool is seen), [4] the head buffer's index.
// ---------------------------------------------------------------------------
constexpr int kPoolTxPk = 5;
constexpr uint32_t kPoolTxMinLog2 = 8;       // every u8 head length fits a buffer (alloc_header's assertion)
constexpr uint32_t kPoolTxOwn = 1u << 31;    // pk[1]: the datagram owns its fragments
constexpr uint32_t kPoolTxHeadFrag = 1u << 31;  // the pass's length row: this fragment is a head
static_assert((1u << kPoolTxMinLog2) >= 255u, "a head fragment lies inside its buffer");
static_assert(15 + 60 <= kRxNS * 16 && 15 + 12 <= kRxNS * 16, "the stash holds the IP header at any start");

// Owner lane, in the pass that holds its head fragment: own = that fragment's stash slot, s = its
// start & 15, hl = its length, L = the datagram's length, wraw = the fragment's raw LE sum, hstart
// = its pool offset.  ipv = the IPv4 header checksum, l4f = the L4 field's offset in the head,
// acc1 = fold(pseudo-header + the head's L4 part with the field as zero), as chain_tx_head and
// csum_txrows_kernel's head() give them.
__device__ __forceinline__ uint8_t pool_tx_head(const CsumArgs &a, const uint4 *own, uint32_t s, uint32_t hl, uint32_t L,
                                                uint32_t wraw, uint64_t hstart, bool present, uint32_t &ipv,
                                                uint32_t &l4f, uint32_t &acc1)
{
    ipv = 0;
    l4f = 0;
    acc1 = 0;
    if (!present)
        return RNS_TX_MALFORMED;
    uint4 ch[kRxNS];
#pragma unroll
    for (int i = 0; i < kRxNS; ++i)
        ch[i] = own[i];  // (a chunk past the fragment's end is stale and never read: every byte used lies below hl)
    uint32_t h[10];
    head40<kRxNS>(ch, s, h);
    uint32_t hdr, field, seed;
    bool v4;
    if (!tx_parse(h, L, hl, hdr, field, seed, v4))
        return RNS_TX_MALFORMED;
    const uint8_t *own8 = reinterpret_cast<const uint8_t *>(own);
    // a byte's share of a LE word sum paired by address (k = its distance from the 16-byte boundary)
    auto le_byte = [](uint32_t b, uint32_t k) { return b << ((k & 1u) * 8u); };
    const int lo = static_cast<int>(s);
    const bool odd = (s & 1u) != 0;
    const uint32_t H = stash_sum_le(ch, lo, lo + static_cast<int>(hdr));
    uint8_t st = 0;
    if (v4) {
        const uint32_t k = s + 10u;
        const uint32_t c = le_byte(own8[k], k) + le_byte(own8[k + 1u], k + 1u);
        ipv = finalize_bits(H - c, odd, false, 0u, true, RNS_FLAG_COMPLEMENT);
        st |= RNS_TX_IP_FILLED;
    }
    if (field != kNoField && L - hdr >= field + 2 && hdr + field + 2 <= hl) {
        l4f = hdr + field;
        const uint32_t k = s + l4f;
        uint32_t b0, b1;
        if (k + 2u <= 16u * kRxNS) {
            b0 = own8[k];
            b1 = own8[k + 1u];
        } else {  // past the stash: the field's two bytes from the pool (inside the head fragment)
            b0 = a.arena[hstart + l4f];
            b1 = a.arena[hstart + l4f + 1u];
        }
        const uint32_t x = fold16(wraw - H - le_byte(b0, k) - le_byte(b1, k + 1u));
        const uint32_t t = seed + (odd ? x : bswap16_u32(x));  // util.rs:89-103 with in_checksum = seed
        acc1 = (t & 0xffff) + (t >> 16);
        st |= RNS_TX_L4_FILLED;
    }
    return st;
}

template <bool NT, bool BUF, uint32_t KMAX>
__global__ __launch_bounds__(kChainBlock, (rx_chain_occ<NT, BUF, KMAX>())) void tx_pool_kernel(const CsumArgs a)
{
    __shared__ uint32_t pk[kPoolTxPk][KMAX * 64];
    __shared__ uint32_t fl[64];          // the pass's fragment lengths (kPoolTxHeadFrag: a head fragment)
    __shared__ uint32_t vq[KMAX + 1];    // V_q: the wave's virtual fragments before block q
    __shared__ uint32_t bq[KMAX];        // d_blk_first of block q
    __shared__ uint4 st[64 * kRxNS];     // the pass's stash: every fragment's first chunks, by sorted position
    const uint32_t lane = threadIdx.x & 63;
    static_assert(kChainBlock == 64, "one wave per workgroup");
    const uint32_t K = KMAX == 1 ? 1u : a.chain_k;
    const uint32_t bmask = a.align_mask, blog = static_cast<uint32_t>(__popc(bmask)), bbytes = bmask + 1u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.arena), static_cast<short>(0), static_cast<int>(BUF ? buf_records(a) : 0), 0x00020000);
    const uint64_t first_pkt = static_cast<uint64_t>(blockIdx.x) * 64ull * K;  // one batch per wave (launch_tx_pool)
    if (first_pkt >= a.n)
        return;
    const uint32_t base = static_cast<uint32_t>(first_pkt);
    uint32_t V = 0;
    for (uint32_t q = 0; q < K; ++q) {
        const uint64_t p = base + q * 64 + lane;  // (32-bit add: the host caps a.n at 2^32 - 64 * kChainMaxK)
        const bool live = p < a.n;
        const uint32_t pay = live ? a.len16[p] : 0u, hl = live ? a.head_len8[p] : 0u;
        const uint32_t nf = live ? 1u + ((pay + bmask) >> blog) : 0u;  // the head buffer and the payload's
        const uint32_t inc = wave_incl_scan(nf);  // <= 64 * (1 + 2^8)
        const uint32_t blk = (base >> 6) + q;     // wave-uniform
        const uint32_t B = static_cast<uint64_t>(blk) * 64 < a.n ? a.first[blk] : 0u;
        // first_i + nf_i <= n_frags, in 64 bits: d_blk_first is the caller's
        const bool ok = live && static_cast<uint64_t>(B) + inc <= a.n_frags;
        pk[0][q * 64 + lane] = V + (inc - nf);
        pk[1][q * 64 + lane] = ok ? kPoolTxOwn | (pay << 8) | hl : 0u;
        pk[2][q * 64 + lane] = 0u;
        pk[3][q * 64 + lane] = RNS_TX_MALFORMED;  // until the head fragment is parsed
        pk[4][q * 64 + lane] = 0u;
        if (lane == 0) {
            vq[q] = V;
            bq[q] = B;
        }
        V += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(inc), 63));
    }
    if (lane == 0)
        vq[K] = V;
    wave_lds_fence();
    const uint32_t passes = (V + 63) / 64;  // V <= 8 * 64 * 257
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
        for (uint32_t q = 0; q < K; ++q) {  // the head holds hl bytes at its buffer's end, the last payload fragment the remainder
            const uint32_t i = q * 64 + lane;
            const uint32_t d = pk[1][i], f0 = pk[0][i];
            const uint32_t pay = (d >> 8) & 0xffffu, npf = (pay + bmask) >> blog;
            if (d & kPoolTxOwn) {
                if (npf != 0 && f0 + npf - fb < 64u)
                    fl[f0 + npf - fb] = pay - ((pay - 1u) & ~bmask);
                if (f0 - fb < 64u)
                    fl[f0 - fb] = kPoolTxHeadFrag | (d & 0xffu);
            }
        }
        wave_lds_fence();
        const uint32_t fv = have ? fl[lane] : 0u;
        uint32_t d_len = fv & 0xffffu;
        uint64_t d_start = (static_cast<uint64_t>(bi) << blog) + ((fv & kPoolTxHeadFrag) ? bbytes - d_len : 0u);
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
            const uint32_t f0 = pk[0][i], d = pk[1][i];
            const uint32_t pay = (d >> 8) & 0xffffu, hl = d & 0xffu;
            const uint32_t nf = (d & kPoolTxOwn) ? 1u + ((pay + bmask) >> blog) : 0u;
            const uint32_t t = max(f0, fb), hi = min(f0 + nf, fb + 64u);
            const bool act = t < hi;
            if (!__ballot(act))
                continue;
            const int l_lo = act ? static_cast<int>(t - fb) : 0, l_hi = act ? static_cast<int>(hi - fb) - 1 : 0;
            const uint32_t s_hi = static_cast<uint32_t>(__shfl(static_cast<int>(S), l_hi, 64));
            const uint32_t s_lo = static_cast<uint32_t>(__shfl(static_cast<int>(S), max(l_lo, 1) - 1, 64));
            const uint32_t R = s_hi - (l_lo ? s_lo : 0u);
            uint32_t add = R & (kPoolFragBad - 1u);
            uint32_t acc = pk[2][i];
            // the head fragment, the range's first: its sum belongs to the head's fold, not the payload's
            const bool headin = act && f0 >= fb;
            if (__ballot(headin)) {
                const int hsrc = headin ? static_cast<int>(f0 - fb) : 0;
                const uint32_t hraw = static_cast<uint32_t>(__shfl(static_cast<int>(w), hsrc, 64));
                const uint32_t hf = static_cast<uint32_t>(__shfl(static_cast<int>(gp), hsrc, 64));
                const uint32_t hbi = static_cast<uint32_t>(__shfl(static_cast<int>(bi), hsrc, 64));
                if (headin) {
                    const uint64_t hstart = (static_cast<uint64_t>(hbi) << blog) + (bbytes - hl);
                    uint32_t ipv, l4f, acc1;
                    const uint8_t fst = pool_tx_head(a, st + ((hf >> kPoolPosShift) & 63u) * kRxNS, (bbytes - hl) & 15u, hl,
                                                     hl + pay, hraw, hstart, hl != 0 && !(hf & kPoolFragBad), ipv, l4f, acc1);
                    pk[3][i] = fst | (l4f << 8) | (ipv << 16);
                    pk[4][i] = hbi;
                    add -= hf & 0xffffu;
                    acc = acc1 << 16;
                }
            }
            if (act) {
                pk[2][i] = fold16((acc & 0xffffu) + add) | (acc & 0xffff0000u);
                if (R >= kPoolFragBad)
                    pk[3][i] = RNS_TX_MALFORMED;
            }
        }
    }
    wave_lds_fence();
    for (uint32_t q = 0; q < K; ++q) {
        const uint64_t p = base + q * 64 + lane;
        const uint32_t i = q * 64 + lane;
        const uint32_t acc = pk[2][i], info = pk[3][i], hl = pk[1][i] & 0xffu;
        const uint32_t fst = info & 0xffu;
        // the payload's fragments as one more fragment fold after the head's (util.rs:112-119): they
        // start 16-byte aligned, so their LE sum swaps to the big-endian one
        const uint32_t t = (acc >> 16) + bswap16_u32(acc & 0xffffu);
        const uint32_t r = ((t & 0xffff) + (t >> 16)) ^ 0xffffu;
        const bool okp = p < a.n && !(fst & RNS_TX_MALFORMED);
        const uint64_t hstart = (static_cast<uint64_t>(pk[4][i]) << blog) + (bbytes - hl);
        // set_be16 into header_mut(): the L4 field, then ip.rs:158-159's IPv4 header checksum
        if (okp && (fst & RNS_TX_L4_FILLED))
            store_field<BUF, RNS_STREAM_OUT_AUX>(a, rsrc, hstart + ((info >> 8) & 0xffu), r);
        if (okp && (fst & RNS_TX_IP_FILLED))
            store_field<BUF, RNS_STREAM_OUT_AUX>(a, rsrc, hstart + 10u, info >> 16);
        if (p < a.n && a.status)
            a.status[p] = static_cast<uint8_t>(fst);  // 64 consecutive bytes per wave
    }
}

}  // namespace rns
