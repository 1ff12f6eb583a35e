// The per-flow state of the TCP receive walks and the blocks of tcp_input's step that the flow update
// (rns_k_flow.hpp) and the connection update (rns_k_conn.hpp) share: the data branch (tcp.rs:642-652), the
// delayed-ACK branch (tcp.rs:654-687), the ACK field (tcp.rs:698-740).  Plain integer C++, no wave intrinsics, no LDS: a host compiler takes it
// (tests/cpp/test_conn_step.cpp).
#pragma once

#include "rns_checksum.h"
#include "rns_k_tcp_head.hpp"

namespace rns {

constexpr uint32_t kFlowDw = 10, kFlowResDw = 6, kFlowMaxFlows = 0x7fffffffu;  // (flow indices stay below 2^31)
constexpr uint32_t kStopNone = 0, kStopMany = 1, kStopState = 2, kStopFlags = 3, kStopOptions = 4, kStopOutside = 5,
                   kStopPend = 6, kStopTwice = 7;
static_assert(kStopMany == RNS_STOP_MANY && kStopState == RNS_STOP_STATE && kStopFlags == RNS_STOP_FLAGS &&
                  kStopOptions == RNS_STOP_OPTIONS && kStopOutside == RNS_STOP_OUTSIDE && kStopPend == RNS_STOP_PEND &&
                  kStopTwice == RNS_STOP_TWICE,
              "rns_checksum.h's stop reasons");

RNS_HD bool seq_gt(uint32_t a, uint32_t b)  // util.rs:155-158
{
    const uint32_t d = a - b;
    return d < 0x80000000u && d != 0u;
}
RNS_HD bool seq_lt(uint32_t a, uint32_t b) { return seq_gt(b, a); }
RNS_HD bool seq_le(uint32_t a, uint32_t b) { return !seq_gt(a, b); }

struct FlowState {  // rns_tcp_flow, and the result's sums
    uint32_t rcv_nxt, rcv_max, snd_una, snd_nxt, snd_wnd, snd_wl1, snd_wl2, rq_len, n_pend, dack_misc;
    uint32_t readable, acked, n_acks, events;
};

RNS_HD void flow_load(FlowState &s, const uint32_t *r)
{
    s.rcv_nxt = r[0];
    s.rcv_max = r[1];
    s.snd_una = r[2];
    s.snd_nxt = r[3];
    s.snd_wnd = r[4];
    s.snd_wl1 = r[5];
    s.snd_wl2 = r[6];
    s.rq_len = r[7];
    s.n_pend = r[8];
    s.dack_misc = r[9];  // delayed_acks | state << 16 | ack_timer << 24
    s.readable = s.acked = s.n_acks = s.events = 0u;
}

RNS_HD void flow_store(const FlowState &s, uint32_t *r)
{
    r[0] = s.rcv_nxt;
    r[1] = s.rcv_max;
    r[2] = s.snd_una;
    r[3] = s.snd_nxt;
    r[4] = s.snd_wnd;
    r[5] = s.snd_wl1;
    r[6] = s.snd_wl2;
    r[7] = s.rq_len;
    r[8] = s.n_pend;
    r[9] = s.dack_misc;
}

RNS_HD void flow_result(const FlowState &s, uint32_t *r, uint32_t n_segs, uint32_t consumed, uint32_t stop, uint32_t why)
{
    r[0] = n_segs;
    r[1] = consumed;
    r[2] = stop;
    r[3] = s.readable;
    r[4] = s.acked;
    r[5] = (s.n_acks & 0xffffu) | (s.events << 16) | (why << 24);
}

// send_packet's window (tcp.rs:403)
RNS_HD uint32_t flow_rcv_window(const FlowState &s) { return (0xffffu - (s.rq_len & 0xffffu)) & 0xffffu; }

// The data branch's head (tcp.rs:642-652), pay > 0: receive_next_seq, add_packet over the pending list
// (pend_cap pairs; seq == rcv_nxt or n_pend < pend_cap on entry), the receive queue's length.
RNS_HD void flow_data_rx(FlowState &s, uint32_t *pend, uint32_t seq, uint32_t pay)
{
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
}

// The delayed-ACK branch of an Established socket (tcp.rs:654-687); force = the segment carries FIN
// (tcp.rs:656).  Returns RNS_SEG_ACK (an immediate ACK: the caller records it), RNS_SEG_TIMER (the timer
// was started) or 0.
RNS_HD uint32_t flow_delayed_ack(FlowState &s, bool force)
{
    uint32_t dack = ((s.dack_misc & 0xffffu) + 1u) & 0xffffu;
    uint32_t timer = s.dack_misc >> 24, did = 0u;
    if (dack >= 5u || force) {  // MAX_DELAYED_ACKS: send_packet, tcp.rs:403-417
        dack = 0u;
        timer = 0u;
        did = RNS_SEG_ACK;
        s.n_acks += 1u;
    } else if (timer == 0u) {
        timer = 1u;
        did = RNS_SEG_TIMER;
    }
    s.dack_misc = dack | (s.dack_misc & 0x00ff0000u) | (timer << 24);
    return did;
}

// The ACK field (tcp.rs:698-740).
RNS_HD void flow_ack_field(FlowState &s, uint32_t seq, uint32_t ack, uint32_t window)
{
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

// The stop that holds before a flow's first segment, if any (n_segs > 0).
RNS_HD uint32_t flow_stop_first(const FlowState &s, uint32_t n_segs, uint32_t pend_cap)
{
    if (n_segs > RNS_FLOW_MAX_SEGS)
        return kStopMany;
    if (((s.dack_misc >> 16) & 0xffu) != RNS_TCP_ESTABLISHED || s.n_pend > pend_cap)
        return kStopState;
    return kStopNone;
}

}  // namespace rns
