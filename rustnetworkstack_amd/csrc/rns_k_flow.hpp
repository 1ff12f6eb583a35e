// TCP flow update (rns_rx_tcp_flow_update_dev) and ACK build (rns_tx_ack_build_dev): tcp_input's
// Established path over the placement's meta records, and the pure ACKs it sends.
// (The kernels of k_flow.hip alone: they are no templates.  Their arguments are in rns_k_args.hpp.)
#pragma once

#include "rns_k_args.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// The update is a per-flow sequential walk (tcp.rs:642-740 is a state machine: every segment's step
// reads the state the one before left), so the work is to give every flow its datagrams in batch
// order.  Grid-wide ordering comes from separate launches on the one stream only; no kernel waits
// on another workgroup.
//   1. flow_count_kernel    a lane per datagram: cnt[flow] += 1 (an integer atomic) for the flow's
//                           datagrams, a zero d_seg record for every other datagram.
//   2. scan (three launches, rns_k_scan.hpp) the exclusive prefix sum of cnt into cursor.
//   3. flow_scatter_kernel  a lane per datagram: list[cursor[flow]++] = its index.  The order within
//                           a flow's list is whatever the atomics gave.
//   4. flow_walk_lane_kernel  a lane per flow, for the flows with at most one datagram (no order to
//                           restore): the 2^20-flows-one-segment-each extreme is one coalesced pass.
//      flow_walk_wave_kernel  a wave per flow, for the others (the scan's second component numbers them, the
//                           cursor kernel lists them, and a grid of at most kFlowWaveGrid waves strides
//                           over the list: no wave is launched for a flow the lane kernel has done): the
//                           wave sorts the flow's (at most
//                           RNS_FLOW_MAX_SEGS) indices ascending in LDS (a bitonic network: the result
//                           is the batch order's whatever the scatter did), loads the four dwords of
//                           each record the step reads into LDS, coalesced over the sorted list, and
//                           lane 0 runs the step loop out of LDS; the wave then writes the flow's
//                           d_seg records from LDS.  The loop is the sequential tail: a step is a few
//                           dependent LDS reads, so 1024 steps cost tens of microseconds whatever
//                           the rest of the wave does, and all flows' loops run side by side.
// Both walks run flow_step, the restatement of the reference's Established step, with the
// pending list in the flow's d_pend_out range (global memory: it is touched only by out-of-order arrivals).
// The walk frames (rns_k_flow_walk.hpp) and the lists' launches (launch_flow_lists) also serve the
// connection update (rns_k_conn.hpp), whose datagram records have four dwords: the step's kRecDw says which.
//
// The ACK build's ACK k is the k-th datagram in batch order with RNS_SEG_ACK: the same scan over the
// pairs (ACKs, IPv4 ACKs), and the consumer kernel builds the heads (rns_k_tcp_head.hpp).
// ---------------------------------------------------------------------------
// --- the flows' lists ---
// A datagram is on flow f's list iff place & RNS_PLACE_FLOW and flow == f < n_flows.
__device__ __forceinline__ uint32_t flow_of(const uint32_t *meta, uint64_t p, uint32_t n_flows)
{
    const uint32_t f = meta[p * 6], place = meta[p * 6 + 5] >> 24;
    return ((place & RNS_PLACE_FLOW) && f < n_flows) ? f : RNS_RX_NO_FLOW;
}

template <uint32_t RecDw>
__device__ __forceinline__ void flow_count(const FlowArgs &a)
{
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    if (p >= a.n_pkts)
        return;
    const uint32_t f = flow_of(a.meta, p, a.n_flows);
    if (f != RNS_RX_NO_FLOW) {
        atomicAdd(a.cnt + f, 1u);
    } else {
#pragma unroll
        for (uint32_t d = 0; d < RecDw; ++d)
            a.rec[RecDw * p + d] = 0u;
    }
}

__global__ __launch_bounds__(kScanBlock) void flow_count_kernel(const FlowArgs a) { flow_count<2>(a); }
// the same for the connection update's four-dword records (k_conn.hip's launch_conn_update asks for it)
__global__ __launch_bounds__(kScanBlock) void flow_count4_kernel(const FlowArgs a) { flow_count<4>(a); }

struct FlowCountValue {
    __device__ static uint2 value(const FlowArgs &a, uint64_t i)
    {
        const uint32_t c = a.cnt[i];
        return make_uint2(c, c > 1u ? 1u : 0u);  // its datagrams; whether the wave walk takes it
    }
};

__global__ __launch_bounds__(kScanBlock) void flow_cursor_kernel(const FlowArgs a)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    const uint2 v = i < a.n_flows ? FlowCountValue::value(a, i) : make_uint2(0u, 0u);
    uint2 total;
    const uint2 ex = scan2_block(v, total);
    if (i < a.n_flows) {
        const uint2 base = a.part[blockIdx.x];
        a.cursor[i] = base.x + ex.x;
        if (v.y)
            a.longs[base.y + ex.y] = static_cast<uint32_t>(i);  // below the count of such flows, <= n_flows
    }
}

__global__ __launch_bounds__(kScanBlock) void flow_scatter_kernel(const FlowArgs a)
{
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    if (p >= a.n_pkts)
        return;
    const uint32_t f = flow_of(a.meta, p, a.n_flows);
    if (f == RNS_RX_NO_FLOW)
        return;
    const uint32_t at = atomicAdd(a.cursor + f, 1u);
    if (at < a.n_pkts)  // always, while d_meta is what the count saw
        a.list[at] = static_cast<uint32_t>(p);
}
// --- the step and the walks ---
// The flow update keeps its own flow_step and walk frames, written out here: built of the shared blocks of
// rns_k_flow_step.hpp under the frames of rns_k_flow_walk.hpp (as the connection update's are) the same logic
// compiled to a wave walk whose loop read 9 % slower on 1024-segment flows (799 against 734 us, alternating
// rounds in one session).  The state, its load / store / result and seq_gt / seq_lt / seq_le are the shared ones.
// One segment: the stop that holds before it, or kStopNone and its step (tcp.rs:642-740 with state ==
// Established); ack_num and wa = window | act << 16 are its d_seg record.  pend = the flow's pending
// list, pend_cap pairs (s.n_pend <= pend_cap on entry, and after).
__device__ __forceinline__ uint32_t flow_step(FlowState &s, uint32_t *pend, uint32_t pend_cap, uint32_t seq, uint32_t ack,
                                              uint32_t win_pay, uint32_t misc, uint32_t &ack_num, uint32_t &wa)
{
    const uint32_t flags = misc & 0xffu, tcp_hdr = (misc >> 16) & 0xffu, place = misc >> 24;
    const uint32_t window = win_pay & 0xffffu, pay = win_pay >> 16;
    if (flags & 0x07u)
        return kStopFlags;
    if (tcp_hdr != 20u)
        return kStopOptions;
    if (place & RNS_PLACE_OUTSIDE)
        return kStopOutside;
    if (pay != 0u && seq != s.rcv_nxt && s.n_pend >= pend_cap)
        return kStopPend;
    ack_num = 0u;
    wa = RNS_SEG_CONSUMED << 16;
    if (pay != 0u) {
        const uint32_t end = seq + pay;
        s.rcv_max = seq_gt(s.rcv_max, end) ? s.rcv_max : end;  // util.rs:172
        uint32_t got = 0u;
        if (seq == s.rcv_nxt) {  // add_packet, tcp.rs:488-516
            got = pay;
            s.rcv_nxt += pay;
            uint32_t i = 0;
            while (i < s.n_pend) {
                const uint32_t ps = pend[2 * i];
                const bool before = seq_gt(seq, ps);
                if (before || ps == s.rcv_nxt) {
                    const uint32_t ln = pend[2 * i + 1];
                    for (uint32_t k = i + 1; k < s.n_pend; ++k) {  // Vec::remove: the tail moves down
                        pend[2 * k - 2] = pend[2 * k];
                        pend[2 * k - 1] = pend[2 * k + 1];
                    }
                    s.n_pend -= 1u;
                    if (!before) {
                        s.rcv_nxt += ln;
                        got += ln;
                        i = 0;
                    }
                } else {
                    i += 1u;
                }
            }
        } else {
            pend[2 * s.n_pend] = seq;
            pend[2 * s.n_pend + 1] = pay;
            s.n_pend += 1u;
        }
        s.rq_len += got;
        s.readable += got;
        uint32_t dack = ((s.dack_misc & 0xffffu) + 1u) & 0xffffu;
        uint32_t timer = s.dack_misc >> 24;
        if (dack >= 5u) {  // MAX_DELAYED_ACKS: send_packet, tcp.rs:403-417
            dack = 0u;
            timer = 0u;
            ack_num = s.rcv_nxt;
            wa = ((0xffffu - (s.rq_len & 0xffffu)) & 0xffffu) | ((RNS_SEG_CONSUMED | RNS_SEG_ACK) << 16);
            s.n_acks += 1u;
        } else if (timer == 0u) {
            timer = 1u;
            wa = (RNS_SEG_CONSUMED | RNS_SEG_TIMER) << 16;
        }
        s.dack_misc = dack | (s.dack_misc & 0x00ff0000u) | (timer << 24);
    }
    if (flags & 0x10u) {  // tcp.rs:698-740
        if (seq_lt(s.snd_una, ack) && seq_le(ack, s.snd_nxt)) {
            s.acked += ack - s.snd_una;
            s.snd_una = ack;
        }
        // (as selects on one flag: written as a branch around the three assignments, with the || and && of
        // the reference, the compiler's branch merging lost snd_wl2 = ack on the snd_wl1 == seq path)
        const uint32_t inside = static_cast<uint32_t>(seq_le(s.snd_una, ack)) & static_cast<uint32_t>(seq_le(ack, s.snd_nxt));
        const uint32_t same = static_cast<uint32_t>(s.snd_wl1 == seq) & static_cast<uint32_t>(seq_le(s.snd_wl2, ack));
        const bool upd = (inside & (static_cast<uint32_t>(seq_lt(s.snd_wl1, seq)) | same)) != 0u;
        s.snd_wnd = upd ? window : s.snd_wnd;
        s.snd_wl1 = upd ? seq : s.snd_wl1;
        s.snd_wl2 = upd ? ack : s.snd_wl2;
        s.events |= upd ? RNS_EV_WND : 0u;
    }
    return kStopNone;
}

// The flow's pending list into its out range: the entries the walk may read.
__device__ __forceinline__ void pend_copy(const FlowArgs &a, uint64_t f, uint32_t n_pend, uint32_t first, uint32_t step)
{
    const uint32_t n = 2u * min(n_pend, a.pend_cap);
    const uint64_t base = 2ull * f * a.pend_cap;
    for (uint32_t k = first; k < n; k += step)
        a.pend_out[base + k] = a.pend_in[base + k];
}

// --- a lane per flow: the flows with at most one datagram ---
__global__ __launch_bounds__(kScanBlock) void flow_walk_lane_kernel(const FlowArgs a)
{
    const uint64_t f = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    if (f >= a.n_flows)
        return;
    const uint32_t n_segs = a.cnt[f];
    if (n_segs > 1u)
        return;
    FlowState s;
    flow_load(s, a.flow_in + f * kFlowDw);
    pend_copy(a, f, s.n_pend, 0u, 1u);
    uint32_t consumed = 0, stop = 0xffffffffu, why = kStopNone;
    if (n_segs == 1u) {
        const uint32_t at = a.cursor[f] - 1u;  // the scatter has moved the cursor to the list's end
        const uint32_t p = at < a.n_pkts ? min(a.list[at], a.n_pkts - 1u) : 0u;
        const uint32_t *m = a.meta + static_cast<uint64_t>(p) * 6;
        uint32_t ack_num = 0, wa = 0;
        why = flow_stop_first(s, n_segs, a.pend_cap);
        if (why == kStopNone)
            why = flow_step(s, a.pend_out + 2ull * f * a.pend_cap, a.pend_cap, m[1], m[2], m[4], m[5], ack_num, wa);
        if (why == kStopNone) {
            consumed = 1u;
        } else {
            stop = p;
            ack_num = wa = 0u;
        }
        a.rec[2ull * p] = ack_num;
        a.rec[2ull * p + 1] = wa;
    }
    flow_store(s, a.flow_out + f * kFlowDw);
    flow_result(s, a.res + f * kFlowResDw, n_segs, consumed, stop, why);
}

// --- a wave per flow: the flows with two datagrams or more ---
constexpr uint32_t kFlowWaveGrid = 4096;  // waves: 20 KiB of LDS each, eight to a CU

__device__ __forceinline__ void flow_walk_wave(const FlowArgs &a, uint32_t f, uint32_t lane,
                                               uint32_t (&idx)[RNS_FLOW_MAX_SEGS], uint32_t (&fld)[4][RNS_FLOW_MAX_SEGS])
{
    const uint32_t n_segs = a.cnt[f];
    if (n_segs <= 1u)
        return;
    const uint32_t end = a.cursor[f];
    // (inside the list whatever the workspace holds)
    const uint32_t first = (end <= a.n_pkts && n_segs <= end) ? end - n_segs : 0u;
    const uint32_t n_list = min(n_segs, a.n_pkts - first);
    FlowState s;
    flow_load(s, a.flow_in + static_cast<uint64_t>(f) * kFlowDw);
    pend_copy(a, f, s.n_pend, lane, 64u);
    uint32_t why = flow_stop_first(s, n_segs, a.pend_cap);
    uint32_t consumed = 0, stop = 0xffffffffu;
    if (why == kStopMany) {  // nothing consumed: zero records, and the flow's first datagram
        uint32_t lo = 0xffffffffu;
        for (uint32_t k = lane; k < n_list; k += 64u) {
            const uint32_t p = min(a.list[first + k], a.n_pkts - 1u);
            a.rec[2ull * p] = 0u;
            a.rec[2ull * p + 1] = 0u;
            lo = min(lo, p);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
            lo = min(lo, static_cast<uint32_t>(__shfl_xor(static_cast<int>(lo), m, 64)));
        stop = lo;
    } else {
        // the list, ascending: a bitonic network over the next power of two, the padding sorts last
        uint32_t N = 2;
        while (N < n_list)
            N <<= 1;
        for (uint32_t k = lane; k < N; k += 64u)
            idx[k] = k < n_list ? min(a.list[first + k], a.n_pkts - 1u) : 0xffffffffu;
        wave_lds_fence();
        for (uint32_t size = 2; size <= N; size <<= 1) {
            for (uint32_t j = size >> 1; j > 0; j >>= 1) {
                for (uint32_t t = lane; t < (N >> 1); t += 64u) {
                    const uint32_t i = 2u * t - (t & (j - 1u));
                    const uint32_t x = idx[i], y = idx[i + j];
                    if ((x > y) == ((i & size) == 0u)) {
                        idx[i] = y;
                        idx[i + j] = x;
                    }
                }
                wave_lds_fence();
            }
        }
        for (uint32_t k = lane; k < n_list; k += 64u) {
            const uint32_t *m = a.meta + static_cast<uint64_t>(idx[k]) * 6;
            fld[0][k] = m[1];
            fld[1][k] = m[2];
            fld[2][k] = m[4];
            fld[3][k] = m[5];
        }
        wave_lds_fence();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // the pending list's copy, the wave's stores, is lane 0's to read
        if (lane == 0) {
            uint32_t *pend = a.pend_out + 2ull * f * a.pend_cap;
            uint32_t k = 0;
            for (; k < n_list && why == kStopNone; ++k) {
                uint32_t ack_num, wa;
                why = flow_step(s, pend, a.pend_cap, fld[0][k], fld[1][k], fld[2][k], fld[3][k], ack_num, wa);
                if (why != kStopNone)
                    break;
                fld[0][k] = ack_num;
                fld[2][k] = wa;
            }
            consumed = k;
            if (why != kStopNone)
                stop = idx[k];
        }
        consumed = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(consumed)));
        wave_lds_fence();
        for (uint32_t k = lane; k < n_list; k += 64u) {
            const uint32_t p = idx[k];
            a.rec[2ull * p] = k < consumed ? fld[0][k] : 0u;
            a.rec[2ull * p + 1] = k < consumed ? fld[2][k] : 0u;
        }
    }
    if (lane == 0) {
        flow_store(s, a.flow_out + static_cast<uint64_t>(f) * kFlowDw);
        flow_result(s, a.res + static_cast<uint64_t>(f) * kFlowResDw, n_segs, consumed, stop, why);
    }
}

__global__ __launch_bounds__(64) void flow_walk_wave_kernel(const FlowArgs a)
{
    __shared__ uint32_t idx[RNS_FLOW_MAX_SEGS];
    __shared__ uint32_t fld[4][RNS_FLOW_MAX_SEGS];  // seq, ack, window | pay_len << 16, flags | .. | place << 24
    const uint32_t n_long = min(a.part[scan_blocks(a.n_flows)].y, a.n_flows);  // the scan's total
    for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        flow_walk_wave(a, min(a.longs[i], a.n_flows - 1u), threadIdx.x, idx, fld);
        wave_lds_fence();  // the next flow reuses the arrays
    }
}

// --- the ACK build ---
// (ACK, IPv4 ACK) of datagram p: an ACK iff its d_seg record says so and its flow is one of the
// flows; an IPv4 one (it takes an id) iff its flow's head length is 40.
struct AckValue {
    __device__ static uint2 value(const AckArgs &a, uint64_t p)
    {
        const uint32_t act = (a.seg[2 * p + 1] >> 16) & 0xffu, f = a.meta[6 * p];
        if (!(act & RNS_SEG_ACK) || f >= a.n_flows)
            return make_uint2(0u, 0u);
        return make_uint2(1u, a.head_len8[f] == 40u ? 1u : 0u);
    }
};

__global__ __launch_bounds__(kScanBlock) void ack_build_kernel(const AckArgs a)
{
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    const uint2 v = p < a.n_pkts ? AckValue::value(a, p) : make_uint2(0u, 0u);
    uint2 total;
    const uint2 ex = scan2_block(v, total);
    if (!v.x)
        return;
    const uint2 base = a.part[blockIdx.x];
    const uint32_t k = base.x + ex.x;
    if (k >= a.ack_cap)
        return;
    const uint32_t f = a.meta[6 * p], hl = a.head_len8[f];
    const uint8_t *t = a.tmpl + static_cast<uint64_t>(f) * a.tmpl_stride;
    const bool v4 = hl == 40u, ok = tcp_tmpl_ok(t, hl, a.tmpl_stride);
    a.ack_src[k] = static_cast<uint32_t>(p);
    a.ack_len8[k] = ok ? static_cast<uint8_t>(hl) : static_cast<uint8_t>(0);
    if (!ok)
        return;
    const uint32_t id = (a.ip_id_base + base.y + ex.y) & 0xffffu;
    const uint32_t seq = a.flow[static_cast<uint64_t>(f) * kFlowDw + 3], ack = a.seg[2 * p];
    const uint32_t window = a.seg[2 * p + 1] & 0xffffu;
    tcp_ctl_head_store(reinterpret_cast<uint32_t *>(a.out + 64ull * k), t, v4, hl, id, seq, ack, window, 0x10u);
}

}  // namespace rns
