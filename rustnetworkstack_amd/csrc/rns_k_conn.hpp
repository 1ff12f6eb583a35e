// TCP connection update (rns_rx_tcp_conn_update_dev), control-segment build (rns_tx_tcp_ctl_build_dev) and
// close step (rns_tx_tcp_close_dev): tcp_input's handshake and close (tcp.rs:622-835), send_packet's
// FIN-aware ACK number (tcp.rs:408-417) and tcp_close (tcp.rs:195-224).
//
// The update is the flow update's decomposition with a wider step: the count, scan, cursor and scatter
// launches (launch_flow_lists, k_flow.hip) and both walk frames (rns_k_flow_walk.hpp) as they are, over
// ConnStepOp.  conn_step is plain integer C++ (a host compiler takes it: tests/cpp/test_conn_step.cpp) and
// calls the flow update's data, delayed-ACK and ACK-field blocks (rns_k_flow_step.hpp).  The wave frame's
// LDS stays 20 KiB: the record's seq takes the slot of the segment's ack, consumed by then.
//
// Unpinned: the reference's trim_head assert (buf.rs:297) trips when acked exceeds the retransmit queue,
// which the SynReceived record's snd_una (the peer's sequence number) makes reachable; the step just counts.
#pragma once

#include "rns_k_flow_step.hpp"

namespace rns {

constexpr uint32_t kTcpFin = 0x01u, kTcpSyn = 0x02u, kTcpRst = 0x04u, kTcpAck = 0x10u;

RNS_HD uint32_t conn_state(const FlowState &s) { return (s.dack_misc >> 16) & 0xffu; }

// set_state (tcp.rs:449-456)
RNS_HD void conn_set_state(FlowState &s, uint32_t state, uint32_t &act)
{
    s.dack_misc = (s.dack_misc & 0xff00ffffu) | (state << 16);
    s.events |= RNS_EV_STATE;
    act |= RNS_CTL_STATE;
}

// send_packet's ack_seq (tcp.rs:408-417) in the state the socket has now.
RNS_HD uint32_t conn_ack_seq(const FlowState &s)
{
    const uint32_t st = conn_state(s);
    const bool fin = (st == RNS_TCP_FIN_WAIT1) | (st == RNS_TCP_FIN_WAIT2) | (st == RNS_TCP_CLOSING) | (st == RNS_TCP_CLOSE_WAIT);
    return s.rcv_nxt + ((fin && s.rcv_max == s.rcv_nxt) ? 1u : 0u);
}

// send_packet(NetBuffer::new(), flags) into a record's fields: out = (ack_num, seq, window | flags << 16).
RNS_HD void conn_send(const FlowState &s, uint32_t flags, uint32_t (&out)[3])
{
    out[0] = conn_ack_seq(s);
    out[1] = s.snd_nxt;
    out[2] = flow_rcv_window(s) | (flags << 16);
}

// One segment: the stop that holds before it, or kStopNone and its step; out = (ack_num, seq, window |
// flags << 16 | act << 24), the record's dwords 2, 1 and 3.  pend as in flow_step.
RNS_HD uint32_t conn_step(FlowState &s, uint32_t *pend, uint32_t pend_cap, uint32_t seq, uint32_t ack, uint32_t win_pay,
                          uint32_t misc, uint32_t (&out)[3])
{
    const uint32_t flags = misc & 0xffu, tcp_hdr = (misc >> 16) & 0xffu, place = misc >> 24;
    const uint32_t window = win_pay & 0xffffu, pay = win_pay >> 16;
    const uint32_t st = conn_state(s);
    const bool fin = (flags & kTcpFin) != 0u, has_ack = (flags & kTcpAck) != 0u;
    const bool acks_fin = has_ack && ack == s.snd_nxt + 1u;
    if (st >= RNS_TCP_SYN_SENT)  // SYN_SENT, LISTEN, and what is no state
        return kStopState;
    if (tcp_hdr != 20u)
        return kStopOptions;
    if (!(flags & kTcpRst)) {
        if ((flags & kTcpSyn) && pay != 0u)
            return kStopFlags;
        if (place & RNS_PLACE_OUTSIDE)
            return kStopOutside;
        if (pay != 0u && seq != s.rcv_nxt && s.n_pend >= pend_cap)
            return kStopPend;
        if (pay != 0u && fin && (st == RNS_TCP_FIN_WAIT2 || (st == RNS_TCP_FIN_WAIT1 && !acks_fin)))
            return kStopTwice;
    }
    uint32_t act = RNS_CTL_CONSUMED;
    out[0] = out[1] = out[2] = 0u;
    if (flags & kTcpRst) {  // A: tcp.rs:635-640
        conn_set_state(s, RNS_TCP_CLOSED, act);
        out[2] = (act | RNS_CTL_RESET) << 24;
        return kStopNone;
    }
    if (pay != 0u) {  // B: tcp.rs:642-696
        flow_data_rx(s, pend, seq, pay);
        if (st == RNS_TCP_ESTABLISHED) {
            const uint32_t did = flow_delayed_ack(s, fin);
            if (did == RNS_SEG_ACK) {
                conn_send(s, kTcpAck, out);
                act |= RNS_CTL_SEND;
            } else if (did) {
                act |= RNS_CTL_ACK_TIMER;
            }
        } else {
            s.dack_misc &= 0x00ffffffu;  // tcp.rs:689-692: the delayed-ACK timer is cancelled
            conn_send(s, kTcpAck, out);
            act |= RNS_CTL_SEND;
            s.n_acks += 1u;
        }
    }
    if (has_ack && st != RNS_TCP_CLOSED && st != RNS_TCP_TIME_WAIT)  // C: tcp.rs:698-740, is_established()
        flow_ack_field(s, seq, ack, window);
    // D: tcp.rs:742-835 (acks_fin was taken with the snd_nxt the arms see: B and C leave it alone)
    if (st == RNS_TCP_SYN_RECEIVED) {
        if (has_ack) {
            conn_set_state(s, RNS_TCP_ESTABLISHED, act);
            s.snd_nxt += 1u;  // the SYN consumes a sequence number
            s.snd_una = ack;
        }
    } else if (st == RNS_TCP_ESTABLISHED) {
        if (fin)
            conn_set_state(s, RNS_TCP_CLOSE_WAIT, act);
    } else if (st == RNS_TCP_LAST_ACK) {
        if (has_ack)
            conn_set_state(s, RNS_TCP_CLOSED, act);
    } else if (st == RNS_TCP_FIN_WAIT1) {
        if (acks_fin && fin) {
            conn_set_state(s, RNS_TCP_TIME_WAIT, act);
            act |= RNS_CTL_TIMEWAIT;
        } else if (fin) {
            conn_set_state(s, RNS_TCP_CLOSING, act);
            conn_send(s, kTcpAck, out);
            act |= RNS_CTL_SEND | RNS_CTL_RESP_TIMER;
            s.n_acks += 1u;
        } else if (acks_fin) {
            conn_set_state(s, RNS_TCP_FIN_WAIT2, act);
        }
    } else if (st == RNS_TCP_FIN_WAIT2) {
        if (fin) {
            conn_send(s, kTcpAck, out);
            act |= RNS_CTL_SEND | RNS_CTL_RESP_TIMER | RNS_CTL_TIMEWAIT;
            s.n_acks += 1u;
            conn_set_state(s, RNS_TCP_TIME_WAIT, act);
        }
    } else if (st == RNS_TCP_CLOSING) {
        if (has_ack) {
            conn_set_state(s, RNS_TCP_TIME_WAIT, act);
            act |= RNS_CTL_TIMEWAIT;
        }
    }
    out[2] |= act << 24;
    return kStopNone;
}

// The stop that holds before a flow's first segment, if any (n_segs > 0); the state is looked at per
// segment, in conn_step.
RNS_HD uint32_t conn_stop_first(const FlowState &s, uint32_t n_segs, uint32_t pend_cap)
{
    if (n_segs > RNS_FLOW_MAX_SEGS)
        return kStopMany;
    return s.n_pend > pend_cap ? kStopState : kStopNone;
}

// tcp_close (tcp.rs:195-224): whether the flow sends; then ctl = its record's four dwords and s its new state.
RNS_HD bool conn_close(FlowState &s, uint32_t f, uint32_t (&ctl)[4])
{
    const uint32_t st = conn_state(s);
    if (st != RNS_TCP_ESTABLISHED && st != RNS_TCP_CLOSE_WAIT)
        return false;
    uint32_t out[3], act = RNS_CTL_SEND | RNS_CTL_RESP_TIMER;
    conn_send(s, kTcpFin | kTcpAck, out);  // before the state change (tcp.rs:211-213, 217-219)
    conn_set_state(s, st == RNS_TCP_ESTABLISHED ? RNS_TCP_FIN_WAIT1 : RNS_TCP_LAST_ACK, act);
    ctl[0] = f;
    ctl[1] = out[1];
    ctl[2] = out[0];
    ctl[3] = out[2] | (act << 24);
    return true;
}

struct ConnStepOp {
    static constexpr uint32_t kRecDw = 4;
    RNS_HD static uint32_t first(const FlowState &s, uint32_t n_segs, uint32_t pend_cap) { return conn_stop_first(s, n_segs, pend_cap); }
    RNS_HD static uint32_t step(FlowState &s, uint32_t *pend, uint32_t pend_cap, uint32_t seq, uint32_t ack, uint32_t win_pay,
                                uint32_t misc, uint32_t &ack_num, uint32_t &seq_out, uint32_t &last)
    {
        uint32_t out[3];
        const uint32_t why = conn_step(s, pend, pend_cap, seq, ack, win_pay, misc, out);
        ack_num = out[0];
        seq_out = out[1];
        last = out[2];
        return why;
    }
};

}  // namespace rns

#ifdef __HIPCC__
#include "rns_k_flow_walk.hpp"

namespace rns {

// --- the walks over the connection update's step ---
__global__ __launch_bounds__(kScanBlock) void conn_walk_lane_kernel(const FlowArgs a) { flow_walk_lane<ConnStepOp>(a); }

__global__ __launch_bounds__(64) void conn_walk_wave_kernel(const FlowArgs a)
{
    __shared__ uint32_t idx[RNS_FLOW_MAX_SEGS];
    __shared__ uint32_t fld[4][RNS_FLOW_MAX_SEGS];  // seq, ack -> the send's seq, window | pay_len << 16, flags | .. | place << 24
    flow_walk_waves<ConnStepOp>(a, idx, fld);
}

// --- the control-segment build ---
// (segment, IPv4 segment) of record i: a segment iff act has RNS_CTL_SEND and its flow is one of the
// flows; an IPv4 one (it takes an id) iff its flow's head length is 40.
struct CtlValue {
    __device__ static uint2 value(const CtlArgs &a, uint64_t i)
    {
        const uint32_t act = a.ctl[4 * i + 3] >> 24, f = a.ctl[4 * i];
        if (!(act & RNS_CTL_SEND) || f >= a.n_flows)
            return make_uint2(0u, 0u);
        return make_uint2(1u, a.head_len8[f] == 40u ? 1u : 0u);
    }
};

__global__ __launch_bounds__(kScanBlock) void ctl_build_kernel(const CtlArgs a)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    const uint2 v = i < a.n_ctl ? CtlValue::value(a, i) : make_uint2(0u, 0u);
    uint2 total;
    const uint2 ex = scan2_block(v, total);
    if (!v.x)
        return;
    const uint2 base = a.part[blockIdx.x];
    const uint32_t k = base.x + ex.x;
    if (k >= a.out_cap)
        return;
    const uint32_t f = a.ctl[4 * i], hl = a.head_len8[f], wfa = a.ctl[4 * i + 3], flags = (wfa >> 16) & 0xffu;
    const uint8_t *t = a.tmpl + static_cast<uint64_t>(f) * a.tmpl_stride;
    const bool v4 = hl == 40u, ok = tcp_tmpl_ok(t, hl, a.tmpl_stride) && !(flags & kTcpSyn);  // (a SYN needs the MSS option)
    a.src[k] = static_cast<uint32_t>(i);
    a.len8[k] = ok ? static_cast<uint8_t>(hl) : static_cast<uint8_t>(0);
    if (!ok)
        return;
    const uint32_t id = (a.ip_id_base + (a.ip_id_add ? *a.ip_id_add : 0u) + base.y + ex.y) & 0xffffu;
    tcp_ctl_head_store(reinterpret_cast<uint32_t *>(a.out + 64ull * k), t, v4, hl, id, a.ctl[4 * i + 1], a.ctl[4 * i + 2],
                       wfa & 0xffffu, flags);
}

// --- the close step: a lane per flow ---
__global__ __launch_bounds__(kScanBlock) void conn_close_kernel(const CloseArgs a)
{
    const uint64_t f = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    if (f >= a.n_flows)
        return;
    FlowState s;
    flow_load(s, a.flow_in + f * kFlowDw);
    uint32_t ctl[4] = {0u, 0u, 0u, 0u};
    if (a.op[f] == 1u)
        conn_close(s, static_cast<uint32_t>(f), ctl);
    flow_store(s, a.flow_out + f * kFlowDw);
    for (uint32_t d = 0; d < 4u; ++d)
        a.ctl[4 * f + d] = ctl[d];
}

}  // namespace rns
#endif
