// TCP send planning (rns_tx_tcp_plan_dev): tcp_write's window gate and retransmit on the device,
// over the flow records the update left, into the descriptors rns_tx_segment_dev takes.
// (The kernels of k_plan.hip alone: they are no templates.  Their arguments are in rns_k_args.hpp.)
#pragma once

#include "rns_k_args.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// tcp_write (tcp.rs:256-292) sends pieces of min(remaining, send_mss) while the piece's end is not
// past send_unacked + send_window; retransmit (tcp.rs:329-348) sends the first send_mss bytes of the
// retransmit queue; both build their head in send_packet (tcp.rs:402-447).  Inside the domain of the
// header (every quantity at most 0x3fffffff) no seq_gt wraps and the loop has a closed form:
//   room  = snd_wnd - inflight (0 when the window has shrunk below what is in flight)
//   full  = min(unsent / mss, room / mss) whole pieces, and the tail piece when every whole piece
//           went and the tail fits what is left of the room.
// Flow f owns entries 2f (the retransmit) and 2f + 1 (the new data) of the segmentation form.
// Grid-wide ordering comes from launch boundaries on the one stream only:
//   1. plan_flow_kernel    a lane per flow: the stops and both entries' byte and segment counts into
//                          a 16-byte record of the workspace.
//   2. scan2_reduce_kernel / scan2_parts_kernel (rns_k_scan.hpp) over the E = 2 n_flows entries: the
//                          pair (segments, IPv4 segments) per 256-entry block.  An entry with segments has
//                          a head of 40 (IPv4) or 60 bytes, so the head bytes before an entry are
//                          60 * segments - 20 * IPv4 segments: three prefixes from one pass.  The
//                          entries' counts enter the scan clamped to seg_cap + 1, which decides the
//                          cap alike and keeps one entry from wrapping the sum.
//   3. plan_cap_kernel     one workgroup: the kept totals.  The kept entries are a prefix; the entry
//                          that crosses seg_cap lies in the last block whose prefix is within the
//                          cap (a binary search over the block prefixes), and that block is scanned
//                          again to find it.  Writes d_n and d_seg_first[E].
//   4. plan_finish_kernel  a lane per flow: scans its block again, applies the cap, writes the
//                          descriptors, results, flow records and the patched template rows, and
//                          fills d_blk_flow — an entry that owns more than one 64-segment block is
//                          spread over its wave.
// ---------------------------------------------------------------------------
// (segments, IPv4 segments) of entry e, the count clamped to seg_cap + 1
struct PlanValue {
    __device__ static uint2 value(const PlanArgs &a, uint64_t e)
    {
        const uint2 r0 = a.rec[e & ~1ull], r1 = a.rec[e | 1ull];
        const uint32_t n = min((e & 1) ? r1.x : (r0.x ? 1u : 0u), a.seg_cap + 1u);  // (seg_cap <= RNS_CHAIN_MAX_PACKETS)
        return make_uint2(n, (r1.y & 0x100u) ? n : 0u);
    }
};

__global__ __launch_bounds__(kScanBlock) void plan_flow_kernel(const PlanArgs a)
{
    const uint64_t f = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    if (f >= a.n_flows)
        return;
    const uint32_t *r = a.flow_in + f * kFlowDw;
    const uint32_t una = r[2], nxt = r[3], wnd = r[4], state = (r[9] >> 16) & 0xffu;
    const uint32_t sq_len = a.sq_len[f], mss = a.mss[f], hl = a.head_len8[f];
    const uint32_t inflight = nxt - una, av = una - a.sq_seq[f];
    uint32_t why = kPlanNone, rex = 0, bytes = 0, segs = 0, v4 = 0;
    if (state != RNS_TCP_ESTABLISHED) {
        why = kPlanState;
    } else if (mss == 0u || sq_len > kPlanMax || wnd > kPlanMax || inflight > kPlanMax || av > sq_len ||
               av + inflight > sq_len) {
        why = kPlanBad;
    } else if (!tcp_tmpl_ok(a.tmpl + f * a.tmpl_stride, hl, a.tmpl_stride)) {
        why = kPlanTmpl;
    } else {
        v4 = hl == 40u ? 1u : 0u;
        if (a.rexmit && a.rexmit[f] && inflight)  // tcp.rs:338-342: one piece from the queue's front
            rex = min(mss, inflight);
        const uint32_t unsent = sq_len - av - inflight;
        const uint32_t room = wnd > inflight ? wnd - inflight : 0u;
        const uint32_t nfull = unsent / mss, kf = min(nfull, room / mss);
        bytes = kf * mss;
        segs = kf;
        if (kf < nfull) {  // the next whole piece is past the window
            why = kPlanWindow;
        } else if (unsent > bytes) {  // the tail piece
            if (unsent - bytes <= room - bytes) {
                bytes = unsent;
                segs += 1u;
            } else {
                why = kPlanWindow;
            }
        }
    }
    a.rec[2 * f] = make_uint2(rex, bytes);
    a.rec[2 * f + 1] = make_uint2(segs, why | (v4 << 8));
}

__global__ __launch_bounds__(kScanBlock) void plan_cap_kernel(const PlanArgs a)
{
    __shared__ uint2 kept;
    const uint64_t E = 2ull * a.n_flows;
    const uint32_t nb = static_cast<uint32_t>(scan_blocks(E));
    const uint2 total = a.part[nb];
    if (threadIdx.x == 0)
        kept = total.x <= a.seg_cap ? total : make_uint2(0u, 0u);
    if (total.x > a.seg_cap) {  // (one value for the workgroup)
        uint32_t lo = 0, hi = nb - 1u;  // the last block whose prefix is within the cap: part[0].x == 0
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1u) / 2u;
            if (a.part[mid].x <= a.seg_cap)
                lo = mid;
            else
                hi = mid - 1u;
        }
        const uint2 base = a.part[lo];
        const uint64_t e = static_cast<uint64_t>(lo) * kScanBlock + threadIdx.x;
        const uint2 v = e < E ? PlanValue::value(a, e) : make_uint2(0u, 0u);
        uint2 sum;
        const uint2 ex = scan2_block(v, sum);  // (its barriers order thread 0's store above before the one below)
        const uint32_t S = base.x + ex.x;
        if (e < E && S <= a.seg_cap && static_cast<uint64_t>(S) + v.x > a.seg_cap)  // the entry that crosses: one lane
            kept = make_uint2(S, base.y + ex.y);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint2 k = kept;
        a.part[nb + 1u] = k;
        a.n_out[0] = k.x;
        a.n_out[1] = k.y;
        a.seg_first[E] = k.x;
    }
}

// Bytes [0, hl) of an entry's row: 16-byte chunks at a 16-byte-aligned row, dwords at a 4-byte-aligned
// one, bytes otherwise (hl is 40 or 60).
__device__ __forceinline__ void plan_row(const uint8_t *t, uint8_t *o, uint32_t hl, uint32_t id, uint32_t seq, uint32_t ack,
                                         uint32_t window)
{
    const bool v4 = hl == 40u;
    const uint32_t nd = hl >> 2, ipd = v4 ? 5u : 10u;
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(o)) & 15u;
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) {
        uint32_t q[4];
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint32_t k = 4u * c + i;
            uint32_t d = 0;
            if (k < nd) {
                __builtin_memcpy(&d, t + 4u * k, 4);
                d = tcp_head_patch(k, d, v4, ipd, id, seq, ack, window, 0x18u, false);
            }
            q[i] = d;
        }
        if (4u * c + 4u <= nd && mis == 0u) {
            *reinterpret_cast<uint4 *>(o + 16u * c) = make_uint4(q[0], q[1], q[2], q[3]);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                const uint32_t k = 4u * c + i;
                if (k >= nd)
                    continue;
                store_dword(o + 4u * k, q[i], (mis & 3u) == 0u);
            }
        }
    }
}

// d_blk_flow of the wave's kept entries: entry e with segments [S, S + n) names the 64-segment blocks
// that start inside it, cnt of them from b0.  A lane writes a single block itself; an entry with more
// (up to 2^24 of them) is spread over the wave.  Every block lies below (seg_cap + 63) / 64: a kept
// entry ends at or before seg_cap.
__device__ __forceinline__ void plan_blocks(const PlanArgs &a, uint32_t lane, uint32_t e, uint32_t b0, uint32_t cnt)
{
    if (cnt == 1u)
        a.blk_flow[b0] = e;
    uint64_t big = __ballot(cnt > 1u);
    while (big) {
        const int l = __ffsll(static_cast<unsigned long long>(big)) - 1;
        big &= big - 1u;
        const uint32_t B0 = static_cast<uint32_t>(__shfl(static_cast<int>(b0), l, 64));
        const uint32_t C = static_cast<uint32_t>(__shfl(static_cast<int>(cnt), l, 64));
        const uint32_t id = static_cast<uint32_t>(__shfl(static_cast<int>(e), l, 64));
        for (uint32_t k = lane; k < C; k += 64u)
            a.blk_flow[B0 + k] = id;
    }
}

__global__ __launch_bounds__(kScanBlock) void plan_finish_kernel(const PlanArgs a)
{
    const uint64_t f = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    const bool live = f < a.n_flows;
    const uint32_t E = 2u * a.n_flows, nb = static_cast<uint32_t>(scan_blocks(E)), cap = a.seg_cap;
    const uint2 kept = a.part[nb + 1u];
    const uint32_t N = min(kept.x, cap);  // (the cap kernel's total is within the cap: a bound whatever the workspace holds)

    // the blocks at and past the kept total name no entry
    const uint32_t nblk = (cap + 63u) >> 6;
    for (uint64_t b = ((N + 63u) >> 6) + f; b < nblk; b += static_cast<uint64_t>(gridDim.x) * kScanBlock)
        a.blk_flow[b] = E;

    // the flow's record and its entries' prefixes
    uint32_t rex = 0, bytes = 0, segs = 0, why = 0, n0 = 0, n1 = 0;
    bool v4 = false;
    if (live) {
        const uint2 r0 = a.rec[2 * f], r1 = a.rec[2 * f + 1];
        rex = r0.x;
        bytes = r0.y;
        segs = r1.x;
        why = r1.y & 0xffu;
        v4 = (r1.y & 0x100u) != 0u;
        n0 = min(rex ? 1u : 0u, cap + 1u);  // as PlanValue
        n1 = min(segs, cap + 1u);
    }
    const uint32_t both = n0 + n1;  // <= cap + 2: no wrap
    uint2 sum;
    const uint2 ex = scan2_block(make_uint2(both, v4 ? both : 0u), sum);
    const uint2 base = live ? a.part[2u * blockIdx.x] : make_uint2(0u, 0u);  // 512 entries: two of the scan's blocks
    const uint32_t S0 = base.x + ex.x, S1 = S0 + n0;
    const uint32_t V0 = base.y + ex.y, V1 = V0 + (v4 ? n0 : 0u);
    const bool keep0 = n0 && static_cast<uint64_t>(S0) + n0 <= cap;
    const bool keep1 = n1 && static_cast<uint64_t>(S1) + n1 <= cap;
    // an entry after the one that crossed the cap lies at the kept totals
    const uint32_t s0 = min(S0, N), s1 = min(S1, N);
    const uint32_t v0 = S0 > N ? kept.y : V0, v1 = S1 > N ? kept.y : V1;

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e0 = 2u * static_cast<uint32_t>(f), e1 = e0 + 1u;
    // (S + n <= cap <= RNS_CHAIN_MAX_PACKETS for a kept entry: + 63 does not wrap)
    const uint32_t b00 = (S0 + 63u) >> 6, b01 = (S1 + 63u) >> 6;
    const uint32_t c0 = keep0 ? ((S0 + n0 + 63u) >> 6) - b00 : 0u, c1 = keep1 ? ((S1 + n1 + 63u) >> 6) - b01 : 0u;
    plan_blocks(a, lane, e0, b00, c0);
    plan_blocks(a, lane, e1, b01, c1);
    if (!live)
        return;

    const uint32_t *r = a.flow_in + f * kFlowDw;
    const uint32_t una = r[2], nxt = r[3];
    const uint32_t hl = a.head_len8[f], mss = a.mss[f];
    const uint64_t q0 = a.sq_off[f] + static_cast<uint32_t>(una - a.sq_seq[f]);  // the byte of snd_una
    const uint32_t new_bytes = keep1 ? bytes : 0u;
    a.pay_off[e0] = keep0 ? q0 : 0u;
    a.pay_off[e1] = keep1 ? q0 + static_cast<uint32_t>(nxt - una) : 0u;
    a.pay_len[e0] = keep0 ? rex : 0u;
    a.pay_len[e1] = new_bytes;
    a.mss_out[e0] = static_cast<uint16_t>(mss);
    a.mss_out[e1] = static_cast<uint16_t>(mss);
    a.head_len8_out[e0] = static_cast<uint8_t>(hl);
    a.head_len8_out[e1] = static_cast<uint8_t>(hl);
    a.seg_first[e0] = s0;
    a.seg_first[e1] = s1;
    a.head_off[e0] = a.head_first_off + 60ull * s0 - 20ull * v0;
    a.head_off[e1] = a.head_first_off + 60ull * s1 - 20ull * v1;

    uint32_t *res = a.res + f * kPlanResDw;
    res[0] = new_bytes;
    res[1] = keep1 ? segs : 0u;
    res[2] = keep0 ? rex : 0u;
    res[3] = (n1 && !keep1) ? kPlanCap : why;
    uint32_t *fo = a.flow_out + f * kFlowDw;
#pragma unroll
    for (uint32_t k = 0; k < kFlowDw; ++k)
        fo[k] = k == 3u ? nxt + new_bytes : r[k];

    if (keep0 || keep1) {
        const uint32_t id0 = a.ip_id_base + (a.ip_id_add ? *a.ip_id_add : 0u);
        const uint32_t window = (0xffffu - (r[7] & 0xffffu)) & 0xffffu;
        const uint8_t *t = a.tmpl + f * a.tmpl_stride;
        if (keep0)
            plan_row(t, a.tmpl_out + static_cast<uint64_t>(e0) * a.tmpl_stride, hl, (id0 + v0) & 0xffffu, nxt, r[0], window);
        if (keep1)
            plan_row(t, a.tmpl_out + static_cast<uint64_t>(e1) * a.tmpl_stride, hl, (id0 + v1) & 0xffffu, nxt, r[0], window);
    }
}

}  // namespace rns
