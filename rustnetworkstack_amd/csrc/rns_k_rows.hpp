// The rows kernels of the plain checksum: packed checksum and fill, and the strided tiny kernel.
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_stream.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// Row stream with owner captures (round 4; the packed form's plain checksum for
// 16-byte-aligned packets above the tiny class: c3, c4, IMIX).
//
// A wave owns 64 consecutive packets and streams their bytes as ONE region, row k =
// the region's k-th KiB (64 lanes x 16 B), D rows in flight — as csum_stream_kernel,
// without its per-row LDS table.  The loading lanes know nothing about packets: each
// sums its whole chunk (4 v_sad_u16), and one DPP scan per row gives the region's
// inclusive prefix P at every chunk.  Packet p (chunks c0..e, 16-aligned start) needs
// only two of those prefixes and its own end chunk:
//     sum_p = P(e - 1) - P(c0 - 1) + (the first ((len - 1) & 15) + 1 bytes of chunk e)
// (P(-1) = 0; e == c0: the end chunk alone).  The owner lane pulls P(c0 - 1) and
// P(e - 1) from the lanes that hold them with ds_bpermute in the rows they fall in, and
// loads its end chunk itself one group of D rows before the row that streams it (the line
// is fetched once), so the end chunk's padding bytes never need a per-row mask.  Rows start
// at the 128-byte line below the region and lanes past its end load nothing.  Per KiB: 4 sad + the scan + two captures, no LDS memory, no fences
// (csum_stream_kernel: a table publish, two wave fences, the masks; 57 VALU/KB).
// u32 differences are exact: a packet's LE word sum is < 2^32.
// ---------------------------------------------------------------------------
// Rows in flight D: 8 at 8 waves/SIMD, or 16 at 4 waves/SIMD for MTU-sized and longer packets
// (c3 isolated 230.2-231.0 -> 227.8-227.9 us; IMIX 445.6-447.6 -> 454-456, so IMIX keeps 8;
// D = 12 at 5 waves/SIMD in between; two or four 64-packet sets per wave slower on IMIX:
// session r04g).
//
// FILL (transmit in-place fill of a packed arena, rns_csum_fill_packed_dev): the field
// (2 bytes at packet offset field[p] / field_off) counts as zero (buf.rs:286-288) and
// receives the result big-endian (tcp.rs:970-973).  The owner loads the 32-byte sector
// around its field with its end chunk, takes the field's bytes out of the row sum, and
// rewrites the whole sector when it lies inside the packet (a full-sector write: no
// read-modify-write at the memory side), else stores the two bytes.
#ifndef RNS_ROWS_FILL_OCC  // waves/SIMD bound of the fill form at D = 8 (8 spills its sector registers)
#define RNS_ROWS_FILL_OCC 6
#endif
#ifndef RNS_ROWS_FILL_BLOCK  // bytes of the aligned block around the field the fill loads and rewrites
#define RNS_ROWS_FILL_BLOCK 32
#endif
// (Two-byte stores, nontemporal and sc0|sc1 block stores were measured and cost the same or more:
// profiles/r04_fill_store_ab.json.)
template <bool NT, bool BUF, int D, bool FILL = false>
__global__ __launch_bounds__(64, D >= 16 ? 4 : FILL ? RNS_ROWS_FILL_OCC : 8) void csum_rows_kernel(const CsumArgs a)
{
    const uint32_t lane = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.arena), static_cast<short>(0), static_cast<int>(BUF ? buf_records(a) : 0), 0x00020000);
    const uint64_t recs = buf_records(a);
    const PackedUnit u = packed_unit(a, lane);
    const uint64_t p = u.p, q = u.q, r0 = u.r0, start = u.start();
    const uint32_t len = u.len, excl = u.excl, total = u.total;
    const uint32_t seed = u.seed;
    const bool live = u.live, ok = u.ok(a);
    // transmit fill: the field, the aligned block of FB bytes around it (a.arena is 16-aligned;
    // the block's alignment is absolute) and whether it lies inside the packet
    constexpr uint32_t FB = FILL ? RNS_ROWS_FILL_BLOCK : 16u, FC = FB / 16u;
    uint32_t fo = 0;
    if constexpr (FILL)
        fo = a.field ? static_cast<uint32_t>(a.field[q]) : a.field_off;
    const bool fok = FILL && live && ok && fo <= len && len - fo >= 2u;  // (no u32 wrap for any field_off)
    const uint64_t fpos = start + fo, fch = fpos & ~15ull;
    const uint32_t back = ((static_cast<uint32_t>(reinterpret_cast<uintptr_t>(a.arena) >> 4) +
                            static_cast<uint32_t>(fch >> 4)) & (FC - 1u)) * 16u;
    const uint64_t sec = fch - back;
    const bool sec_ok = fok && fch >= back && sec + FB <= recs;
    const uint32_t rel = static_cast<uint32_t>(fpos - sec);  // the field's first byte in the block
    uint4 sv[FC];
    uint32_t fb0 = 0, fb1 = 0;  // the field's bytes when the block does not hold both
    if constexpr (FILL) {
#pragma unroll
        for (uint32_t i = 0; i < FC; ++i) {
            if constexpr (BUF) {
                const uint32_t o = sec_ok ? static_cast<uint32_t>(sec) + 16u * i : kOobOffset;
                const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o, 0, 0);
                sv[i] = make_uint4(x.x, x.y, x.z, x.w);
            } else {
                sv[i] = sec_ok ? load_chunk<false>(a.arena + sec + 16u * i) : make_uint4(0, 0, 0, 0);
            }
        }
        if (fok && (!sec_ok || rel == FB - 1u)) {  // rare: odd field at a block end, or the arena's first chunk
            fb0 = a.arena[fpos];
            fb1 = a.arena[fpos + 1];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    uint32_t mine = 0;
    bool odd = false;
    if ((r0 & 15) == 0) {
        const uint32_t c0 = excl >> 4;
        const uint32_t e = len ? (excl + len - 1) >> 4 : c0;
        mine = rows_region_sum<NT, BUF, D>(a, rsrc, recs, r0, total, c0, e, len);
    } else {
        // ---- unaligned region (rare): the whole wave sums one packet at a time ----
        // (wave_serial_sums' loop, kept in place: see there)
        const uint64_t start = r0 + excl;
        const bool ok = start <= a.arena_bytes && len <= a.arena_bytes - start;
        uint64_t todo = __ballot(len != 0 && ok);
        while (todo) {
            const uint32_t o = static_cast<uint32_t>(__builtin_ctzll(todo));
            todo &= todo - 1;
            const uint64_t st =
                (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(start >> 32), o)))
                 << 32) |
                static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(start), o));
            const uint32_t L = __builtin_amdgcn_readlane(len, o);
            const Pkt k = make_pkt(st, L);
            uint32_t acc = 0;
            for (uint32_t cc = 0; cc < k.nch; cc += 64) {
                uint4 w[1];
                issue_pass<64, 1, NT, BUF, 1>(a, rsrc, k, cc + lane, w);
                mask_edges<64, 1, 1>(k, cc + lane, w);
                acc = sum_le<1, 1>(w, acc);
            }
            const uint32_t sum = group_allreduce<64>(acc);
            mine = lane == o ? sum : mine;
        }
        odd = r0 & 1;  // every packet of the range shares the region start's misalignment
    }
    if constexpr (FILL) {
        // the field's bytes out of the sum (LE words pair bytes by absolute parity)
        uint32_t w[4 * FC];
#pragma unroll
        for (uint32_t i = 0; i < FC; ++i) {
            w[4 * i] = sv[i].x;
            w[4 * i + 1] = sv[i].y;
            w[4 * i + 2] = sv[i].z;
            w[4 * i + 3] = sv[i].w;
        }
        uint32_t b0 = fb0, b1 = fb1;
        if (sec_ok && rel != FB - 1u) {
            uint32_t d0 = 0, d1 = 0;
#pragma unroll
            for (uint32_t d = 0; d < 4 * FC; ++d) {
                d0 = (rel >> 2) == d ? w[d] : d0;
                d1 = ((rel + 1u) >> 2) == d ? w[d] : d1;
            }
            b0 = (d0 >> ((rel & 3u) * 8u)) & 0xffu;
            b1 = (d1 >> (((rel + 1u) & 3u) * 8u)) & 0xffu;
        }
        mine -= fok ? (b0 << ((fpos & 1) * 8)) + (b1 << (((fpos + 1) & 1) * 8)) : 0u;
        const uint16_t r = finalize_bits(mine, odd, false, seed, ok && fok, a.flags);
        // set_be16(&mut packet[fo..fo + 2], result): rewrite the largest aligned block (FB, ..., 32
        // bytes) around the field that lies inside the packet, else store the two bytes
        const uint32_t hi = static_cast<uint32_t>(r) >> 8, lo = static_cast<uint32_t>(r) & 0xffu;
        uint8_t *arena_w = const_cast<uint8_t *>(a.arena);
        uint32_t wsz = 0;  // bytes of the block rewritten
#pragma unroll
        for (uint32_t bs = 32; bs <= FB; bs *= 2) {
            const uint64_t bb = sec + (rel & ~(bs - 1u));
            wsz = sec_ok && (rel & (bs - 1u)) != bs - 1u && bb >= start && bb + bs <= start + len ? bs : wsz;
        }
        if (wsz) {
#pragma unroll
            for (uint32_t d = 0; d < 4 * FC; ++d) {
                const uint32_t s0 = (rel & 3u) * 8u, s1 = ((rel + 1u) & 3u) * 8u;
                w[d] = (rel >> 2) == d ? (w[d] & ~(0xffu << s0)) | (hi << s0) : w[d];
                w[d] = ((rel + 1u) >> 2) == d ? (w[d] & ~(0xffu << s1)) | (lo << s1) : w[d];
            }
            const uint32_t c_lo = (rel & ~(wsz - 1u)) >> 4, c_hi = c_lo + (wsz >> 4);
#pragma unroll
            for (uint32_t i = 0; i < FC; ++i)
                if (i >= c_lo && i < c_hi)
                    store_block(reinterpret_cast<uint4 *>(arena_w + sec + 16u * i),
                                make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]));
        } else if (fok) {
            arena_w[fpos] = static_cast<uint8_t>(hi);
            arena_w[fpos + 1] = static_cast<uint8_t>(lo);
        }
    }
    const uint16_t res = finalize_bits(mine, odd, false, seed, ok && (!FILL || fok), a.flags);
    if (live && (!FILL || a.out)) {
        if (a.n < (1u << 30)) {  // buffer store, sc0|sc1 (the stream kernel's measured best, r03o)
            const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                static_cast<void *>(a.out), static_cast<short>(0), static_cast<int>(2u * a.n), 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b16(res, out_rsrc, static_cast<uint32_t>(2 * p), 0, RNS_STREAM_OUT_AUX);
        } else {
            __builtin_nontemporal_store(res, a.out + p);
        }
    }
    if (a.bad) {
        const uint64_t rejected = __ballot(live && !(ok && (!FILL || fok)));
        if (rejected && lane == 0)
            atomicAdd(a.bad, static_cast<uint32_t>(__popcll(rejected)));
    }
}

// ---------------------------------------------------------------------------
// Tiny fixed-size packets at a fixed stride (rns_csum_batch_strided_dev, c2: 2^20 x 64 B):
// packet i = arena[first_off + i * stride, + len) with len <= 64 and 16-byte-aligned starts,
// so a packet is at most 4 chunks and a wave's 64 packets are 4 rows of 16 packets x 4 chunks
// whose addresses the lanes compute themselves — no descriptors but the seeds, no per-round
// broadcast (the rounds kernel's fetch_pkt), every row of every batch in flight at once.  A
// quad of lanes sums its packet (two DPP steps); the owner lane pulls its packet's sum with one
// ds_bpermute per row and finishes (util.rs:88-106: the LE sum folded and byte-swapped — the
// starts are even — plus the seed, folded).
// ---------------------------------------------------------------------------
template <bool BUF, int B>
__global__ __launch_bounds__(64) void csum_strided_tiny_kernel(const CsumArgs a)
{
    const uint32_t lane = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.arena), static_cast<short>(0), static_cast<int>(BUF ? buf_records(a) : 0), 0x00020000);
    const uint64_t recs = buf_records(a);
    const uint32_t L = a.fixed_len;  // 1..64
    const uint32_t j = lane & 3u;
    const uint32_t jb = 16u * j;
    const uint64_t start0 = a.first_off + a.base_adjust;
    // the seeds first, with the rows (issued where they are used they cost the wave a second
    // memory latency after its rows: 12.24-12.29 -> 12.06-12.08 us per isolated dispatch, r05m)
    uint32_t sd[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const uint64_t p = (static_cast<uint64_t>(blockIdx.x) * B + b) * 64 + lane;
        sd[b] = 0;
        if (a.seed)
            sd[b] = a.seed[p < a.n ? p : a.n - 1];
    }
    uint4 v[B][4];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const uint64_t base = (static_cast<uint64_t>(blockIdx.x) * B + b) * 64;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t q = base + 16u * r + (lane >> 2);
            const uint64_t o = start0 + q * a.stride + jb;
            v[b][r] = load16<BUF, true>(a, rsrc, o, q < a.n && jb < L && o + 16 <= recs);
        }
    }
    const int src = static_cast<int>((lane & 15u) << 4);  // lane 4 * (p & 15) of the owner's row
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const uint64_t base = (static_cast<uint64_t>(blockIdx.x) * B + b) * 64;
        const uint64_t p = base + lane;
        uint32_t mine = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            uint4 x = v[b][r];
            if (jb + 16u > L)  // the packet's last chunk: its bytes past len never count
                x = jb < L ? keep_first(x, L - jb) : make_uint4(0, 0, 0, 0);
            const uint32_t t = group_allreduce<4>(sad4(x, 0u));
            const uint32_t got = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src, static_cast<int>(t)));
            mine = (lane >> 4) == static_cast<uint32_t>(r) ? got : mine;
        }
        if (p < a.n) {
            const uint64_t st = start0 + p * a.stride;
            const bool ok = st <= a.arena_bytes && L <= a.arena_bytes - st;
            a.out[p] = finalize_bits(mine, false, false, sd[b], ok, a.flags);  // 64 consecutive u16: one 128-byte store
        }
        if (a.bad) {
            const uint64_t st = start0 + p * a.stride;
            const uint64_t rejected = __ballot(p < a.n && !(st <= a.arena_bytes && L <= a.arena_bytes - st));
            if (rejected && lane == 0)
                atomicAdd(a.bad, static_cast<uint32_t>(__popcll(rejected)));
        }
    }
}

}  // namespace rns
