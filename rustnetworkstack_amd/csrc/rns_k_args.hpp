// What every translation unit sees of the entry points that are sequences of launches: their kernel
// arguments, constants and workspace sizes.  Their kernels are no templates, so each family's header is
// included by the one translation unit that launches it (k_flow.hip, k_plan.hip, k_echo.hip, k_udp.hip,
// k_udp_tx.hip, k_listen.hip, k_conn.hip).
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_flow_step.hpp"
#include "rns_k_pool_place.hpp"
#include "rns_k_pool_txform.hpp"
#include "rns_k_scan.hpp"

namespace rns {

// --- the flow update and the ACK build (rns_k_flow.hpp) ---
// (kFlowDw, kFlowResDw, kFlowMaxFlows and the stop reasons: rns_k_flow_step.hpp)
struct FlowArgs {
    const uint32_t *meta;     // 6 dwords per datagram
    const uint32_t *flow_in;  // 10 dwords per flow
    const uint32_t *pend_in;  // pend_cap (seq, len) pairs per flow
    uint32_t *flow_out, *pend_out;
    uint32_t *rec;            // a record per datagram: d_seg's 2 dwords, or the connection update's d_ctl's 4 (the step's kRecDw)
    uint32_t *res;            // 6 dwords per flow
    uint32_t *cnt, *cursor;   // workspace: n_flows each
    uint32_t *longs;          // workspace: n_flows, the flows with two datagrams or more
    uint32_t *list;           // workspace: n_pkts
    uint2 *part;              // workspace: the scan's block sums, blocks + 1
    uint32_t n_pkts, n_flows, pend_cap;
};

// The workspace, 8-byte aligned: the scan's block sums as pairs first (the flows' blocks + 1 for the
// update; the datagrams' blocks + 1 for the ACK build, which uses nothing else and may share the
// update's workspace once the update is done), then cnt, cursor and longs (n_flows dwords each) and
// list (n_pkts).
inline uint64_t flow_work_bytes(uint64_t n_pkts, uint64_t n_flows)
{
    return 4ull * (3 * n_flows + n_pkts + 2 * (scan_blocks(n_flows) + 1) + 2 * (scan_blocks(n_pkts) + 1));
}
inline uint64_t ack_work_bytes(uint64_t n_pkts) { return 8ull * (scan_blocks(n_pkts) + 1); }

struct AckArgs {
    const uint32_t *meta, *seg, *flow;
    const uint8_t *tmpl, *head_len8;
    uint8_t *out;
    uint32_t *ack_src;
    uint8_t *ack_len8;
    uint32_t *n_acks;
    uint2 *part;
    uint32_t n_pkts, n_flows, tmpl_stride, ip_id_base, ack_cap;
};

// --- the connection update, the control-segment build and the close step (rns_k_conn.hpp) ---
// (The update takes FlowArgs with rec = d_ctl and the flow update's workspace.)
constexpr uint32_t kCtlDw = 4;

struct CtlArgs {
    const uint32_t *ctl;       // 4 dwords per record
    const uint8_t *tmpl, *head_len8;
    const uint32_t *ip_id_add;
    uint8_t *out;
    uint32_t *src;
    uint8_t *len8;
    uint32_t *count;
    uint2 *part;               // workspace: the scan's block sums, blocks + 1
    uint32_t n_ctl, n_flows, tmpl_stride, ip_id_base, out_cap;
};

inline uint64_t ctl_work_bytes(uint64_t n_ctl) { return 8ull * (scan_blocks(n_ctl) + 1); }

struct CloseArgs {
    const uint32_t *flow_in;   // 10 dwords per flow
    uint32_t *flow_out;
    const uint8_t *op;
    uint32_t *ctl;             // 4 dwords per flow
    uint32_t n_flows;
};

// --- the send planning (rns_k_plan.hpp) ---
constexpr uint32_t kPlanNone = 0, kPlanWindow = 1, kPlanState = 2, kPlanBad = 3, kPlanTmpl = 4, kPlanCap = 5;
static_assert(kPlanNone == RNS_PLAN_NONE && kPlanWindow == RNS_PLAN_WINDOW && kPlanState == RNS_PLAN_STATE &&
                  kPlanBad == RNS_PLAN_BAD && kPlanTmpl == RNS_PLAN_TMPL && kPlanCap == RNS_PLAN_CAP,
              "rns_checksum.h's plan reasons");
constexpr uint32_t kPlanMax = 0x3fffffffu, kPlanMaxFlows = 1u << 30, kPlanResDw = 4;

struct PlanArgs {
    const uint32_t *flow_in;  // 10 dwords per flow
    uint32_t *flow_out;
    const uint64_t *sq_off;
    const uint32_t *sq_seq, *sq_len;
    const uint16_t *mss;
    const uint8_t *rexmit, *tmpl, *head_len8;
    const uint32_t *ip_id_add;
    uint8_t *tmpl_out, *head_len8_out;
    uint64_t *pay_off;
    uint32_t *pay_len;
    uint16_t *mss_out;
    uint64_t *head_off;
    uint32_t *seg_first, *blk_flow, *n_out;
    uint32_t *res;   // 4 dwords per flow
    uint2 *part;     // workspace: the scan's block sums, blocks + 2 (the total, then the kept total)
    uint2 *rec;      // workspace: two pairs per flow, (rexmit bytes, new bytes), (new segments, why | IPv4 << 8)
    uint64_t head_first_off;
    uint32_t n_flows, tmpl_stride, ip_id_base, seg_cap;
};

// The workspace, 8-byte aligned: the block sums of the E = 2 n_flows entries and two more pairs, then
// the flows' records.
inline uint64_t plan_work_bytes(uint64_t n_flows) { return 8ull * (scan_blocks(2 * n_flows) + 2) + 16ull * n_flows; }

// --- the echo responder (rns_k_echo.hpp) ---
constexpr uint32_t kEchoMinLog2 = 8;  // the transmit pool form's: a head fits its buffer

struct EchoArgs {
    PoolRx rx;
    PoolTx tx;  // (blog = rx.blog: both pools have the same buffer size)
    BuildWork w;
    LocalAddrs local;
    uint8_t *echo;
};

inline uint64_t echo_work_bytes(uint64_t n_pkts) { return build_work_bytes(n_pkts); }

// --- the UDP receive demux (rns_k_udp.hpp) ---
constexpr uint32_t kUdpMinLog2 = 7;  // 60 + 8 header bytes lie inside the first buffer
// A tile is the datagrams of one workgroup: kUdpSteps 64-datagram blocks per wave.  Two keep the grid of
// 2^20 datagrams at 8 workgroups per CU and the counts matrix of 1024 sockets at 16 MiB.
constexpr uint32_t kUdpSteps = 2, kUdpWaves = kScanBlock / 64, kUdpTile = kScanBlock * kUdpSteps;
// the workspace's dword per datagram: socket | payload bytes << 16
constexpr uint32_t kUdpNoSock = RNS_UDP_NO_SOCK, kUdpNotDgram = 0xfffeu;  // both >= RNS_UDP_MAX_SOCKS
static_assert(kUdpNotDgram >= RNS_UDP_MAX_SOCKS && kUdpNoSock >= RNS_UDP_MAX_SOCKS, "no socket index");

struct UdpArgs {
    PoolRx rx;
    const uint16_t *port_tbl;  // 65536 entries
    uint8_t *data;             // 16-byte aligned
    uint64_t data_bytes;
    uint4 *rec_out;            // two per record
    uint32_t *q_first, *count;
    uint8_t *udp;
    uint32_t *pos;             // optional
    uint32_t *rec;             // workspace: a dword per datagram
    uint2 *mat;                // workspace: (entries, units) of socket s in tile t at s * n_tiles + t
    uint2 *part;               // workspace: the scan's block sums over the matrix, blocks + 1
    uint32_t n_socks, n_tiles, rec_cap;
};

inline uint64_t udp_tiles(uint64_t n_pkts) { return (n_pkts + kUdpTile - 1) / kUdpTile; }
// The workspace, 8-byte aligned pieces: the block sums of the M = n_socks * tiles matrix entries, the
// matrix itself (8 B per entry), then the datagrams' dwords.  2^20 datagrams and 1024 sockets: 20 MiB.
inline uint64_t udp_work_bytes(uint64_t n_pkts, uint64_t n_socks)
{
    const uint64_t m = n_socks * udp_tiles(n_pkts);
    return 8ull * (scan_blocks(m) + 1) + 8ull * m + 4ull * n_pkts;
}

// --- the UDP send build (rns_k_udp_tx.hpp) ---
constexpr uint32_t kUdpTxMinLog2 = 8;  // the transmit pool form's: a head fits its buffer

struct UdpTxArgs {
    const uint8_t *data;       // 16-byte aligned: the payloads, record k's at 16 * off16
    uint64_t data_bytes;
    const uint4 *rec_in;       // two per record (rns_udp_rec)
    const uint32_t *q_first;   // n_socks + 1
    const uint16_t *sock_port; // n_socks
    PoolTx tx;
    BuildWork w;
    LocalAddrs local;
    uint8_t *send;
    uint32_t n_recs, n_socks;
};

inline uint64_t udp_tx_work_bytes(uint64_t n_recs) { return build_work_bytes(n_recs); }

// --- the TCP listen responder (rns_k_listen.hpp) ---
struct ListenArgs {
    PoolRx rx;                 // (status is not read: the meta records carry the verify's verdict)
    const uint32_t *meta;      // 6 dwords per datagram
    const uint16_t *listen;    // 65536 entries
    const uint32_t *iss;
    const uint32_t *ip_id_add;
    uint8_t *out;
    uint32_t *rep_src;
    uint8_t *rep_len8;
    uint32_t *accept;          // 18 dwords per record
    uint32_t *count;
    uint8_t *conn;
    BuildWork w;               // workspace: here part_a = (replies, IPv4 replies), part_b = (accepts, 0)
    unsigned long long *tbl;   // workspace: the key table's slots, resident | the key's hash << 32
    uint32_t *first;           // workspace: a slot's smallest candidate index
    uint64_t slots;
    LocalAddrs local;
    uint32_t n_listen, reply_cap, ip_id_base;
};

// Slots of the key table for n_pkts datagrams: the flow table's rule, a power of two >= 2 * n_pkts and >= 64.
// The workspace, 8-byte aligned: the table (8 + 4 B per slot, the two arrays one after the other so that one fill
// clears both; 12 * slots is a multiple of 8), then the build's own.  2^20 datagrams: 28 MiB.
inline uint64_t listen_work_bytes(uint64_t n_pkts)
{
    return build_work_bytes(n_pkts) + 12ull * flow_slots(static_cast<uint32_t>(n_pkts));
}

}  // namespace rns
