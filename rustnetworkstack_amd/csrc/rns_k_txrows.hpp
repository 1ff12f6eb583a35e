// The transmit-shaped chains: the head fragment's finish (chain_tx_head) and csum_txrows_kernel in its
// FILL, FIN and CPT forms.
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_rows_tx.hpp"

namespace rns {

// The head fragment's part of a chain's transmit finalize (csum_txrows_kernel FIN mode): ch =
// the head's chunks from the 16-byte boundary at or below its start (s = start & 15), hl = its
// length (the IP header and, behind it, the L4 header: alloc_header prepends both into one
// fragment, buf.rs:262-291), L = the datagram's length over every fragment.  ipv = the IPv4
// header checksum to store at head + 10 (ip.rs:140-160); l4f = the L4 field's offset in the
// head (kNoField: no L4 fill — a protocol the stack does not checksum, a segment too short
// for its field, or a field past the head fragment); hsum = the LE word sum of the head's L4
// part with the field as zero (valid when s + hl <= 16 * NS); seed = the pseudo-header sum.
// The L4 part starts at an even distance from the head's start (IHL*4 or 40), so hsum pairs
// exactly as that part would alone.
template <int NS>
__device__ __forceinline__ uint8_t chain_tx_head(const uint4 (&ch)[NS], uint32_t s, uint32_t hl, uint32_t L, bool odd,
                                                 bool present, uint32_t &ipv, uint32_t &l4f, uint32_t &hsum,
                                                 uint32_t &seed, uint32_t &hdr)
{
    ipv = 0;
    l4f = kNoField;
    hsum = 0;
    seed = 0;
    hdr = 0;
    if (!present)
        return RNS_TX_MALFORMED;
    uint32_t h[10];
    head40(ch, s, h);
    uint32_t field;
    bool v4;
    if (!tx_parse(h, L, hl, hdr, field, seed, v4))
        return RNS_TX_MALFORMED;
    const int lo = static_cast<int>(s);
    uint8_t st = 0;
    if (v4) {
        const uint32_t H = stash_sum_le(ch, lo, lo + static_cast<int>(hdr)) - stash_sum_le(ch, lo + 10, lo + 12);
        ipv = finalize_bits(H, odd, false, 0u, true, RNS_FLAG_COMPLEMENT);
        st |= RNS_TX_IP_FILLED;
    }
    if (field != kNoField && L - hdr >= field + 2 && hdr + field + 2 <= hl) {
        l4f = hdr + field;
        const int f = lo + static_cast<int>(l4f);
        hsum = stash_sum_le(ch, lo + static_cast<int>(hdr), lo + static_cast<int>(hl)) - stash_sum_le(ch, f, f + 2);
        st |= RNS_TX_L4_FILLED;
    }
    return st;
}

// ---------------------------------------------------------------------------
// Transmit-shaped chains (RNS_FLAG_CHAIN_TX_PACKED; rns_csum_chain_dev and
// rns_csum_chain_fill_dev).  What tcp_output checksums (tcp.rs:938-973) is a head fragment
// (the TCP header alloc_header prepended, buf.rs:262-291) followed by the payload.  A batching
// transmit path keeps the heads of consecutive packets back to back in a header region and the
// payloads back to back, 16-byte aligned, in a payload region.  Then a wave's 64 payloads are
// ONE region and stream as csum_rows_kernel's rows (P(e-1) - P(c0-1) + the owner's end chunk),
// while each owner loads its own head (at most 4 chunks; the 64 heads of a wave are one
// contiguous run, so those loads coalesce) and, for the fill, stores its field into it:
// 64 two-byte stores into one short run of lines instead of 64 scattered writes.
//
// The chain is folded as compute_buffer_ones_comp does (util.rs:112-119): acc = fold(seed +
// G(head)), then fold(acc + G(payload)) — the payload's fragments form a run (back to back,
// even non-final lengths: their words pair as one slice's), so the payload is
// one contiguous sum; G(x) is the folded sum in big-endian order (zero iff all bytes zero).
// With the fill the field's two bytes are taken out of the head's exact sum before the fold.
//
// Every lane classifies its packet from its first 1 + kRunFrags descriptors (one round of
// loads after first[]).  A wave whose packets all have that shape (or a defined rejection:
// malformed range, no fragments, a fragment outside the arena, a head too short for its
// field) and whose payloads ascend at 16-byte starts with bounded gaps takes the rows; any
// other wave takes an exact per-packet loop (the whole wave sums one fragment at a time,
// big-endian words mod 2^32: util.rs:88-106 literally), so the hint never changes a result.
//
// FIN (rns_tx_fill_chain_dev): the whole transmit finalize of such chains — the head fragment
// holds the IP header and the L4 header behind it (alloc_header prepends both into one fragment,
// buf.rs:262-291), so the owner parses its head (chain_tx_head), forms the pseudo-header from the
// head's addresses and the chain's length, sums the head's L4 part, and stores the L4 field and
// the IPv4 header checksum into the head: tcp.rs:957-973, udp.rs:151-171, icmp.rs:87-112,
// ip.rs:140-160 over [head[hdr..], payload...] exactly as compute_buffer_ones_comp folds it.
// Heads of up to 80 bytes from their 16-byte boundary (an IPv6 + TCP head at any start) take
// the rows; the status byte goes to a.status.
//
// CPT (rns_tx_fill_chain_packed_dev): FIN over the compact descriptors of this project's own
// transmit layout — datagram i = [head, payload] with a u8 head length (a.head_len8) and a u16
// payload length (a.len16; 0 = head only), heads back to back from a.head_blk_off[b], payloads
// at multiples of align_mask + 1 from a.blk_off[b] for each 64-datagram block b: 3 B per
// datagram + 16 B per block instead of 28 B.  Only the descriptor round differs: one round of
// loads (no first[] round, no per-fragment loop, no run classification) and two DPP scans give
// the head's and the payload's offsets.  The payloads ascend with bounded gaps by construction,
// so the region test is "the payload block offset is 16-byte aligned", and a wave's heads are
// always one run, so every fast wave without a rejected datagram takes the run write-back.  A
// wave with a head past 80 bytes from its 16-byte boundary or an unaligned payload block takes
// the exact loop, fed from the implied offsets.  From the head chunks on the code is FIN's.
// ---------------------------------------------------------------------------
#ifndef RNS_TXROWS_OCC  // waves/SIMD bound of the transmit-rows kernel
#define RNS_TXROWS_OCC 5  // (zero scratch at 86-89 VGPRs; 6 spills 32-116 B/lane)
#endif
constexpr uint32_t kTxHeadMax = 64;  // (head start & 15) + head length: at most 4 chunks (5 for FIN)
#ifndef RNS_TXFIN_RUN_AUX  // cache-policy bits of the run write-back's chunk stores: nontemporal (c3 277.3 ->
#define RNS_TXFIN_RUN_AUX kNtAux  // 270.1 us cold, IMIX 626.4 -> 624.7; plain stores 282.2 / 634.6: r06t)
#endif
#ifndef RNS_TXFIN_RUNWRITE  // FIN: write a wave's back-to-back heads back as whole chunks
#define RNS_TXFIN_RUNWRITE 1  // (IMIX 652.1-652.2 -> 632.5 us, c3 257.3 -> 256.0 against two 2-byte
#endif                        //  stores per head: session r06h, txops / txops_rw)

template <bool NT, bool BUF, int D, bool FILL, bool FIN = false, bool CPT = false>
__global__ __launch_bounds__(64, RNS_TXROWS_OCC) void csum_txrows_kernel(const CsumArgs a)
{
    static_assert(!(FILL && FIN), "FIN finds its fields itself");
    static_assert(!CPT || FIN, "the compact descriptors are a form of FIN");
    constexpr uint32_t kNH = FIN ? 5u : 4u;  // head chunks the fast path holds
    constexpr uint32_t kHeadMax = 16u * kNH;
    const uint32_t lane = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.arena), static_cast<short>(0), static_cast<int>(BUF ? buf_records(a) : 0), 0x00020000);
    const uint64_t recs = buf_records(a);
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 64 + lane;
    const bool live = p < a.n;
    uint32_t f0 = 0, f1 = 0;
    uint32_t hl8 = 0, pl16 = 0;      // CPT: the lane's two lengths
    uint64_t hblk = 0, pblk = 0;     // CPT: the wave's two block offsets (loaded per lane, as csum_rows_kernel's)
    if constexpr (CPT) {
        // the whole descriptor round: one u8, one u16 and the block's two offsets
        const uint64_t q = live ? p : a.n - 1;  // branch-free descriptor loads
        const uint64_t blk = (p >> 6) + __builtin_amdgcn_mbcnt_lo(0u, 0u);
        hblk = a.head_blk_off[blk];
        pblk = a.blk_off[blk];
        hl8 = live ? static_cast<uint32_t>(a.head_len8[q]) : 0u;
        pl16 = live ? static_cast<uint32_t>(a.len16[q]) : 0u;
        f1 = live ? (pl16 ? 2u : 1u) : 0u;  // the chain [head] or [head, payload]
    } else {
        f0 = live ? a.first[p] : 0u;
        f1 = live ? a.first[p + 1] : 0u;
    }
    const bool rng_ok = CPT || (f0 <= f1 && f1 <= a.n_frags);
    const uint32_t nfr = live && rng_ok ? f1 - f0 : 0u;
    const uint32_t seed = (a.seed && live) ? static_cast<uint32_t>(a.seed[p]) : 0u;
    uint32_t fo = 0;
    if constexpr (FILL)
        fo = live ? (a.field ? static_cast<uint32_t>(a.field[p]) : a.field_off) : 0u;
    // the head and up to kRunFrags payload fragments: one round of descriptor loads
    constexpr uint32_t kF = 1 + kRunFrags;
    uint64_t o[kF];
    uint32_t l[kF];
#pragma unroll
    for (uint32_t j = 0; j < kF; ++j) {
        o[j] = 0;
        l[j] = 0;
        if (!CPT && j < nfr) {
            o[j] = a.off[f0 + j] + a.base_adjust;
            l[j] = a.len[f0 + j];
        }
    }
    bool all_in = true, run = nfr <= kF;
    uint32_t plen = 0;
    uint64_t pbase = 0;  // CPT: the wave's payload block offset
    if constexpr (CPT) {
        // head i starts where head i-1 ends; payload i at the padded end of payload i-1
        const uint32_t ppad = (pl16 + a.align_mask) & ~a.align_mask;
        const uint32_t hin = wave_incl_scan(hl8), pin = wave_incl_scan(ppad);
        pbase = lane_u64(pblk, 0) + a.base_adjust;
        o[0] = lane_u64(hblk, 0) + a.base_adjust + (hin - hl8);
        l[0] = hl8;
        o[1] = pbase + (pin - ppad);
        l[1] = pl16;
        plen = pl16;
        all_in = o[0] <= a.arena_bytes && hl8 <= a.arena_bytes - o[0] &&
                 (pl16 == 0 || (o[1] <= a.arena_bytes && pl16 <= a.arena_bytes - o[1]));
    }
#pragma unroll
    for (uint32_t j = 0; j < kF; ++j) {
        if (!CPT && j < nfr) {
            const bool in = o[j] <= a.arena_bytes && l[j] <= a.arena_bytes - o[j];
            all_in = all_in && in;
            if (j >= 1) {
                run = run && (j == 1 || (o[j] == o[j - 1] + l[j - 1] && !(l[j - 1] & 1u)));
                plen += l[j];
            }
        }
    }
    const uint32_t hl = l[0];
    // defined rejections (every path): bad range, a fragment outside the arena and, for the fill,
    // no fragments or a head too short for the field — the packet gets 0, is counted and is left
    // untouched.  (The checksum of a packet without fragments is its seed, as the reference's
    // loop over no fragments returns initial_sum.)
    bool bad = live && (!rng_ok || (nfr <= kF && !all_in));
    if constexpr (FILL)
        bad = bad || (live && (nfr == 0 || !(fo <= hl && hl - fo >= 2u)));
    if constexpr (FIN)
        bad = bad || (live && nfr == 0);
    const bool has_pay = live && !bad && plen != 0;
    const uint64_t po = o[1];
    const bool shape = !live || bad ||
                       (run && plen <= 0xFFFFu && (o[0] & 15u) + hl <= kHeadMax && (!has_pay || (po & 15u) == 0));
    // the wave's payload region: ascending, 16-byte starts, gaps bounded (else the exact loop)
    const uint64_t pm = __ballot(has_pay);
    uint64_t r0 = 0;
    uint32_t rel = 0, c0 = 0, e = 0, total = 0;
    bool region = true;
    if constexpr (CPT) {
        // the payloads ascend from the block offset with gaps below the alignment: one region
        region = !pm || (pbase & 15u) == 0;
        if (pm) {
            r0 = pbase;
            rel = static_cast<uint32_t>(po - pbase);
            const uint32_t last = 63u - static_cast<uint32_t>(__builtin_clzll(pm));
            total = __builtin_amdgcn_readlane(rel + ((plen + 15u) & ~15u), last);  // the last payload's end
            c0 = has_pay ? rel >> 4 : 0u;
            e = has_pay ? (rel + plen - 1u) >> 4 : 0u;
        }
    } else if (pm) {
        const uint32_t fl = static_cast<uint32_t>(__builtin_ctzll(pm));
        r0 = lane_u64(po, fl);
        const uint64_t rel64 = has_pay ? po - r0 : 0;
        const uint32_t pad = has_pay ? (plen + 15u) & ~15u : 0u;
        const bool near = rel64 < (1ull << 30);
        rel = static_cast<uint32_t>(rel64);
        const uint32_t end = has_pay && near ? rel + pad : 0u;
        const uint32_t incl = wave_incl_max(end);
        const uint32_t before = static_cast<uint32_t>(__shfl(static_cast<int>(incl), static_cast<int>(lane) - 1, 64));
        const bool asc = !has_pay || (near && (lane == 0 || rel >= before));
        total = __builtin_amdgcn_readlane(incl, 63);
        const uint32_t sum_pad = __builtin_amdgcn_readlane(wave_incl_scan(pad), 63);
        region = !__ballot(!asc) && total <= 2u * sum_pad + 4096u;
        c0 = has_pay ? rel >> 4 : 0u;
        e = has_pay ? (rel + plen - 1u) >> 4 : 0u;
    }
    const bool fast = !__ballot(!shape) && region;
    uint32_t res = 0;  // the folded sum (before the complement)
    uint32_t fst = RNS_TX_MALFORMED, ipv = 0, l4f = kNoField;  // FIN: status, IPv4 checksum, L4 field
    // FIN run write-back (RNS_TXFIN_RUNWRITE): a fast wave whose heads lie back to back (one run)
    // stages its raw head chunks in LDS, patches its fields there and writes the run's whole
    // 16-byte chunks back (full 64-byte segments, about half the write requests of two field
    // stores per head); fields in the run's partial edge chunks take the 2-byte stores.
    // (the same write-back for the one-field fill measured no gain: c3 246.8 / IMIX 598.0 us against
    // 246.1 / 597.8, session r06n — its 20-byte heads already leave one request per 64-byte segment)
    constexpr bool kRunWrite = FIN && RNS_TXFIN_RUNWRITE != 0;
    bool runw = false;
    uint64_t b0 = 0, r1 = 0;  // the run's first chunk boundary, its end
    if constexpr (kRunWrite) {
        const uint64_t hend = o[0] + hl;
        const uint64_t pe = lane_below_u64(hend, lane);
        const bool contig = !live || (!bad && (CPT || lane == 0 || o[0] == pe));  // (CPT: by construction)
        runw = fast && !__ballot(!contig);
        const uint32_t last = 63u - static_cast<uint32_t>(__builtin_clzll(__ballot(live)));
        b0 = first_lane_u64(o[0]) & ~15ull;
        r1 = lane_u64(hend, last);
    }
    __shared__ uint4 run_lds[kRunWrite ? 64u * kNH + 1u : 1u];
    if (fast) {
        // the owner's head: its chunks issued before the rows, consumed after the first group
        const uint64_t hb = o[0] & ~15ull;
        const uint32_t hs = static_cast<uint32_t>(o[0] & 15u), span = live && !bad ? hs + hl : 0u;
        uint4 h[kNH];
#pragma unroll
        for (uint32_t i = 0; i < kNH; ++i)
            h[i] = own_chunk<BUF>(a, rsrc, recs, hb, span, i);
        uint32_t acc1 = 0;
        auto head = [&]() {
            uint32_t hsum = 0, sd = seed;
            if constexpr (kRunWrite) {
                if (runw) {  // the raw chunks the head touches (neighbours' bytes in them are raw too)
                    const uint32_t q = static_cast<uint32_t>((hb - b0) >> 4);
#pragma unroll
                    for (uint32_t i = 0; i < kNH; ++i)
                        if (16u * i < span)
                            run_lds[q + i] = h[i];
                }
            }
            if constexpr (FIN) {
                uint32_t hd;
                fst = chain_tx_head<kNH>(h, hs, hl, hl + plen, (o[0] & 1u) != 0, live && !bad, ipv, l4f, hsum, sd, hd);
            } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const int lo = static_cast<int>(hs) - 16 * static_cast<int>(i), hi = static_cast<int>(span) - 16 * static_cast<int>(i);
                hsum = __builtin_amdgcn_sad_u16(keep_bytes(h[i].x, lo, hi, 0), 0, hsum);
                hsum = __builtin_amdgcn_sad_u16(keep_bytes(h[i].y, lo, hi, 4), 0, hsum);
                hsum = __builtin_amdgcn_sad_u16(keep_bytes(h[i].z, lo, hi, 8), 0, hsum);
                hsum = __builtin_amdgcn_sad_u16(keep_bytes(h[i].w, lo, hi, 12), 0, hsum);
            }
            }
            if constexpr (FILL) {  // the field counts as zero (buf.rs:286-288)
                const uint32_t w[16] = {h[0].x, h[0].y, h[0].z, h[0].w, h[1].x, h[1].y, h[1].z, h[1].w,
                                        h[2].x, h[2].y, h[2].z, h[2].w, h[3].x, h[3].y, h[3].z, h[3].w};
                const uint32_t q0 = hs + fo, q1 = q0 + 1u;  // < 64 for a packet that is not rejected
                uint32_t d0 = 0, d1 = 0;
#pragma unroll
                for (uint32_t d = 0; d < 16; ++d) {
                    d0 = (q0 >> 2) == d ? w[d] : d0;
                    d1 = (q1 >> 2) == d ? w[d] : d1;
                }
                const uint32_t b0 = (d0 >> ((q0 & 3u) * 8u)) & 0xffu, b1 = (d1 >> ((q1 & 3u) * 8u)) & 0xffu;
                hsum -= (live && !bad) ? (b0 << ((q0 & 1u) * 8u)) + (b1 << ((q1 & 1u) * 8u)) : 0u;
            }
            const uint32_t x = fold16(hsum);
            const uint32_t g = (o[0] & 1u) ? x : bswap16_u32(x);
            const uint32_t t = sd + g;  // util.rs:89-103 with in_checksum = seed (no wrap: <= 0x1fffe)
            acc1 = (t & 0xffff) + (t >> 16);
        };
        uint32_t mine = 0;
        if (pm) {
            mine = rows_region_sum<NT, BUF, D>(a, rsrc, recs, r0, total, c0, e, has_pay ? plen : 0u, nullptr, head);
        } else {
            head();
        }
        const uint32_t x = fold16(mine);
        const uint32_t t = acc1 + bswap16_u32(x);  // the payload starts 16-byte aligned: even
        res = has_pay ? (t & 0xffff) + (t >> 16) : acc1;
    } else {
        // ---- the exact per-packet loop: the whole wave sums one fragment at a time ----
        uint32_t sd = seed, hd = 0;
        if constexpr (FIN) {
            // the chain's length, and every fragment (not just the first kF) inside the arena
            uint32_t lt = 0;
            bool in = true;
            if constexpr (CPT) {
                lt = hl + plen;  // (both fragments were checked above)
            } else if (live && rng_ok) {
                for (uint32_t f = f0; f < f1; ++f) {
                    const uint64_t so = a.off[f] + a.base_adjust;
                    const uint32_t lf = a.len[f];
                    in = in && so <= a.arena_bytes && lf <= a.arena_bytes - so;
                    lt += lf;
                }
            }
            bad = bad || (live && !in);
            // the head's first 81-96 bytes from its 16-byte boundary: the IP header and the L4 field
            const uint64_t hb = o[0] & ~15ull;
            const uint32_t s0 = static_cast<uint32_t>(o[0] & 15u);
            uint4 own[6];
#pragma unroll
            for (int i = 0; i < 6; ++i)
                own[i] = own_chunk<BUF>(a, rsrc, recs, hb, live && !bad ? s0 + hl : 0u, i);
            uint32_t hsum;
            fst = chain_tx_head<6>(own, s0, hl, lt, (o[0] & 1u) != 0, live && !bad, ipv, l4f, hsum, sd, hd);
        }
        uint64_t todo = FIN ? __ballot(live && !bad && l4f != kNoField) : __ballot(live && rng_ok && nfr != 0 && !bad);
        bool lbad = bad;
        res = sd;  // (a packet without fragments)
        while (todo) {
            const uint32_t ow = static_cast<uint32_t>(__builtin_ctzll(todo));
            todo &= todo - 1;
            const uint32_t F0 = __builtin_amdgcn_readlane(f0, ow), F1 = __builtin_amdgcn_readlane(f1, ow);
            // FIN: the L4 part of the head starts HD bytes in, its field FO bytes after that
            const uint32_t HD = FIN ? __builtin_amdgcn_readlane(hd, ow) : 0u;
            const uint32_t FO = FIN ? __builtin_amdgcn_readlane(l4f, ow) - HD : __builtin_amdgcn_readlane(fo, ow);
            uint32_t acc = __builtin_amdgcn_readlane(sd, ow);
            bool pbad = false;
            // CPT: the owner's implied fragments (F0 = 0: fragment 0 the head, 1 the payload)
            const uint64_t HO = CPT ? lane_u64(o[0], ow) : 0, PO = CPT ? lane_u64(o[1], ow) : 0;
            const uint32_t HL = CPT ? __builtin_amdgcn_readlane(hl, ow) : 0u, PL = CPT ? __builtin_amdgcn_readlane(plen, ow) : 0u;
            for (uint32_t f = F0; f < F1; ++f) {
                uint64_t st;
                uint32_t L;
                if constexpr (CPT) {
                    st = f == 0 ? HO : PO;
                    L = f == 0 ? HL : PL;
                } else {
                    st = a.off[f] + a.base_adjust;
                    L = a.len[f];
                }
                if (!(st <= a.arena_bytes && L <= a.arena_bytes - st)) {
                    pbad = true;
                    break;
                }
                if (FIN && f == F0) {  // the IP header was prepended after the L4 checksum
                    st += HD;
                    L -= HD;
                }
                if (L == 0)  // an empty fragment adds nothing (the reference panics on it)
                    continue;
                const Pkt k = make_pkt(st, L);
                const uint32_t w_hi = (st & 1) ? 0x01000100u : 0x00010001u;
                const uint64_t fpos = st + FO;  // FILL / FIN: the field in the head fragment (f == F0)
                uint32_t hsb = 0, lsb = 0;
                for (uint32_t cc = 0; cc < k.nch; cc += 64) {
                    uint4 w[1];
                    issue_pass<64, 1, NT, BUF, 1>(a, rsrc, k, cc + lane, w);
                    mask_edges<64, 1, 1>(k, cc + lane, w);
                    if ((FILL || FIN) && f == F0) {
                        const uint64_t cs = (st & ~15ull) + (static_cast<uint64_t>(cc + lane) << 4);
                        const int lo = static_cast<int>(static_cast<int64_t>(fpos) - static_cast<int64_t>(cs));
                        if (lo > -2 && lo < 16) {  // zero the field's bytes in this chunk
                            // (keep_bytes keeps [lo, hi) of a dword: here everything but [lo, lo + 2))
                            w[0].x &= ~keep_bytes(0xffffffffu, lo, lo + 2, 0);
                            w[0].y &= ~keep_bytes(0xffffffffu, lo, lo + 2, 4);
                            w[0].z &= ~keep_bytes(0xffffffffu, lo, lo + 2, 8);
                            w[0].w &= ~keep_bytes(0xffffffffu, lo, lo + 2, 12);
                        }
                    }
                    sum_be<1, 1>(w, w_hi, hsb, lsb);
                }
                const uint32_t words = group_allreduce<64>((hsb << 8) + lsb);  // BE words mod 2^32
                acc += words;                                                   // util.rs:89-99
                while (acc > 0xffff)                                            // util.rs:101-103
                    acc = (acc & 0xffff) + (acc >> 16);
            }
            if (lane == ow) {
                res = acc;
                lbad = pbad;
            }
        }
        bad = lbad;
    }
    const bool okp = live && !bad;
    const uint32_t r = (FIN || (a.flags & RNS_FLAG_COMPLEMENT)) ? res ^ 0xffffu : res;
    // the fields to store (set_be16 into header_mut()): FIN the L4 field, then ip.rs:158-159's
    // IPv4 header checksum; FILL the caller's field
    constexpr uint64_t kNoPos = ~0ull;
    uint64_t fpos[2] = {kNoPos, kNoPos};
    uint32_t fval[2] = {0u, 0u};
    if constexpr (FIN) {
        if (okp && (fst & RNS_TX_L4_FILLED)) {
            fpos[0] = o[0] + l4f;
            fval[0] = r;
        }
        if (okp && (fst & RNS_TX_IP_FILLED)) {
            fpos[1] = o[0] + 10;
            fval[1] = ipv;
        }
    }
    if constexpr (FILL) {
        if (okp) {
            fpos[0] = o[0] + fo;
            fval[0] = r;
        }
    }
    uint64_t c0w = 0, c1w = 0;  // the run's whole chunks [c0w, c1w) (run write-back)
    if constexpr (kRunWrite) {
        if (runw) {
            uint8_t *l8 = reinterpret_cast<uint8_t *>(run_lds);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (fpos[k] != kNoPos) {
                    l8[fpos[k] - b0] = static_cast<uint8_t>(fval[k] >> 8);
                    l8[fpos[k] - b0 + 1] = static_cast<uint8_t>(fval[k]);
                }
            }
            __syncthreads();
            c0w = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(o[0] & 15u)) == 0 ? b0 : b0 + 16;
            c1w = r1 & ~15ull;
            uint8_t *w8 = const_cast<uint8_t *>(a.arena);
            for (uint64_t c = c0w + 16u * lane; c < c1w; c += 1024u) {
                const uint4 v = run_lds[(c - b0) >> 4];
                if constexpr (BUF) {
                    const u32x4 y = {v.x, v.y, v.z, v.w};
                    __builtin_amdgcn_raw_buffer_store_b128(y, rsrc, static_cast<uint32_t>(c), 0, RNS_TXFIN_RUN_AUX);
                } else {
                    *reinterpret_cast<uint4 *>(w8 + c) = v;
                }
            }
        }
    }
    // (field stores as buffer stores with the result stores' sc0|sc1 bits: IMIX 604.4 -> 598.4 us,
    // c3 251.0 -> 245.7 against ordinary stores; nontemporal 595.8 / 246.4: session r05e; with the
    // run write-back only the fields not wholly inside its chunks)
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (fpos[k] != kNoPos && (!runw || fpos[k] < c0w || fpos[k] + 2 > c1w))
            store_field<BUF, RNS_STREAM_OUT_AUX>(a, rsrc, fpos[k], fval[k]);
    if constexpr (FIN) {
        if (live && a.status)
            a.status[p] = okp ? static_cast<uint8_t>(fst) : static_cast<uint8_t>(RNS_TX_MALFORMED);
    }
    if (live && a.out) {
        const uint16_t v = okp ? static_cast<uint16_t>(r) : static_cast<uint16_t>(0);
        if (a.n < (1u << 30)) {
            const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                static_cast<void *>(a.out), static_cast<short>(0), static_cast<int>(2u * a.n), 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b16(v, out_rsrc, static_cast<uint32_t>(2 * p), 0, RNS_STREAM_OUT_AUX);
        } else {
            __builtin_nontemporal_store(v, a.out + p);
        }
    }
    count_rejected(a, lane, live && !okp);
}

}  // namespace rns
