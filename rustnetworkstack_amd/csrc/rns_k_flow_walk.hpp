// The two walk frames of a per-flow receive walk over a step Op (ConnStepOp of rns_k_conn.hpp, the connection
// update's; the flow update keeps frames of its own in rns_k_flow.hpp, see there): a lane per flow with at most one
// segment, a wave per longer flow with the sort and the step loop out of LDS.  Device functions only: the
// kernels that call them are in rns_k_conn.hpp.
#pragma once

#include "rns_k_args.hpp"

namespace rns {

// A datagram's record: Op::kRecDw dwords at a.rec.  Two (rns_rx_tcp_seg): ack_num, window | act << 16.
// Four (rns_tcp_ctl): flow, seq, ack_num, window | flags << 16 | act << 24.  o0, o1, o2 = the step's ack_num,
// seq and last dword, f its flow; all zero for a segment that is not consumed.  (The lists' launch writes the other datagrams' zero records with the same Op::kRecDw:
// launch_flow_lists(a, Op::kRecDw), k_flow.hip.)
template <class Op>
__device__ __forceinline__ void walk_record(const FlowArgs &a, uint64_t p, uint32_t f, uint32_t o0, uint32_t o1, uint32_t o2)
{
    if constexpr (Op::kRecDw == 2) {
        a.rec[2ull * p] = o0;
        a.rec[2ull * p + 1] = o2;
    } else {
        uint32_t *r = a.rec + 4ull * p;  // (4-byte aligned like d_seg: dword stores)
        r[0] = f;
        r[1] = o1;
        r[2] = o0;
        r[3] = o2;
    }
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
template <class Op>
__device__ __forceinline__ void flow_walk_lane(const FlowArgs &a)
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
        uint32_t ack_num = 0, seq_out = 0, last = 0;
        why = Op::first(s, n_segs, a.pend_cap);
        if (why == kStopNone)
            why = Op::step(s, a.pend_out + 2ull * f * a.pend_cap, a.pend_cap, m[1], m[2], m[4], m[5], ack_num, seq_out, last);
        if (why == kStopNone) {
            consumed = 1u;
        } else {
            stop = p;
            ack_num = seq_out = last = 0u;
        }
        walk_record<Op>(a, p, consumed ? static_cast<uint32_t>(f) : 0u, ack_num, seq_out, last);
    }
    flow_store(s, a.flow_out + f * kFlowDw);
    flow_result(s, a.res + f * kFlowResDw, n_segs, consumed, stop, why);
}

// --- a wave per flow: the flows with two datagrams or more ---
constexpr uint32_t kFlowWaveGrid = 4096;  // waves: 20 KiB of LDS each, eight to a CU

template <class Op>
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
    uint32_t why = Op::first(s, n_segs, a.pend_cap);
    uint32_t consumed = 0, stop = 0xffffffffu;
    if (why == kStopMany) {  // nothing consumed: zero records, and the flow's first datagram
        uint32_t lo = 0xffffffffu;
        for (uint32_t k = lane; k < n_list; k += 64u) {
            const uint32_t p = min(a.list[first + k], a.n_pkts - 1u);
            walk_record<Op>(a, p, 0u, 0u, 0u, 0u);
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
                uint32_t ack_num, seq_out, last;
                why = Op::step(s, pend, a.pend_cap, fld[0][k], fld[1][k], fld[2][k], fld[3][k], ack_num, seq_out, last);
                if (why != kStopNone)
                    break;
                fld[0][k] = ack_num;  // (the outputs take the slots of inputs already consumed)
                if constexpr (Op::kRecDw == 4)
                    fld[1][k] = seq_out;
                fld[2][k] = last;
            }
            consumed = k;
            if (why != kStopNone)
                stop = idx[k];
        }
        consumed = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(consumed)));
        wave_lds_fence();
        for (uint32_t k = lane; k < n_list; k += 64u) {
            const bool done = k < consumed;
            walk_record<Op>(a, idx[k], done ? f : 0u, done ? fld[0][k] : 0u, done ? fld[1][k] : 0u, done ? fld[2][k] : 0u);
        }
    }
    if (lane == 0) {
        flow_store(s, a.flow_out + static_cast<uint64_t>(f) * kFlowDw);
        flow_result(s, a.res + static_cast<uint64_t>(f) * kFlowResDw, n_segs, consumed, stop, why);
    }
}

// The wave kernel's body: a grid of at most kFlowWaveGrid waves strides over the long flows' list.
template <class Op>
__device__ __forceinline__ void flow_walk_waves(const FlowArgs &a, uint32_t (&idx)[RNS_FLOW_MAX_SEGS],
                                                uint32_t (&fld)[4][RNS_FLOW_MAX_SEGS])
{
    const uint32_t n_long = min(a.part[scan_blocks(a.n_flows)].y, a.n_flows);  // the scan's total
    for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        flow_walk_wave<Op>(a, min(a.longs[i], a.n_flows - 1u), threadIdx.x, idx, fld);
        wave_lds_fence();  // the next flow reuses the arrays
    }
}

}  // namespace rns
