// TCP flow update and ACK build (rns_rx_tcp_flow_update_dev, rns_tx_ack_build_dev): the launch
// sequences — every grid-wide dependency is a launch boundary on the one stream — and the
// workspace's host-side sizing.
#include "rns_launch.hpp"
#include "rns_k_flow.hpp"

namespace rns {

static uint32_t blocks_of(uint64_t n) { return static_cast<uint32_t>(scan_blocks(n)); }

// The launches before the walks: cnt, cursor (moved to each list's end), longs and list are filled, and every
// datagram that is no flow's has its zero record of rec_dw dwords: d_seg's 2, or d_ctl's 4.  The connection update
// (k_conn.hip) starts with the same launches.
int launch_flow_lists(const FlowArgs &a, uint32_t rec_dw, hipStream_t st)
{
    if (rec_dw != 2 && rec_dw != 4)
        return RNS_E_INVALID;
    const auto count = rec_dw == 2 ? flow_count_kernel : flow_count4_kernel;
    if (a.n_flows == 0) {  // every datagram's record is zero
        RNS_LAUNCH(count, blocks_of(a.n_pkts), kScanBlock, st, a);
        return RNS_OK;
    }
    RNS_TRY(launch_fill32(a.cnt, a.n_flows, 0u, st));
    if (a.n_pkts) {
        const uint32_t nb = blocks_of(a.n_flows);
        RNS_LAUNCH(count, blocks_of(a.n_pkts), kScanBlock, st, a);
        RNS_LAUNCH((scan2_reduce_kernel<FlowCountValue, FlowArgs>), nb, kScanBlock, st, a, static_cast<uint64_t>(a.n_flows),
                   a.part);
        RNS_TRY(launch_scan2_parts(a.part, nb, nullptr, st));
        RNS_LAUNCH(flow_cursor_kernel, nb, kScanBlock, st, a);
        RNS_LAUNCH(flow_scatter_kernel, blocks_of(a.n_pkts), kScanBlock, st, a);
    }
    return RNS_OK;
}

int launch_flow_update(const FlowArgs &a, hipStream_t st)
{
    RNS_TRY(launch_flow_lists(a, 2, st));
    if (a.n_flows == 0)
        return RNS_OK;
    RNS_LAUNCH(flow_walk_lane_kernel, blocks_of(a.n_flows), kScanBlock, st, a);
    if (a.n_pkts >= 2)  // a flow with two datagrams exists only then, and at most n_pkts / 2 of them
        RNS_LAUNCH(flow_walk_wave_kernel, std::min({a.n_flows, a.n_pkts / 2, kFlowWaveGrid}), 64, st, a);
    return RNS_OK;
}

int launch_ack_build(const AckArgs &a, hipStream_t st)
{
    if (a.n_pkts == 0)
        return launch_fill32(a.n_acks, 2, 0u, st);
    const uint32_t nb = blocks_of(a.n_pkts);
    RNS_LAUNCH((scan2_reduce_kernel<AckValue, AckArgs>), nb, kScanBlock, st, a, static_cast<uint64_t>(a.n_pkts), a.part);
    RNS_TRY(launch_scan2_parts(a.part, nb, a.n_acks, st));
    if (a.ack_cap)
        RNS_LAUNCH(ack_build_kernel, nb, kScanBlock, st, a);
    return RNS_OK;
}

}  // namespace rns

using namespace rns;

extern "C" int rns_rx_tcp_flow_update_work(uint32_t n_pkts, uint32_t n_flows, uint64_t *bytes)
{
    if (!bytes || n_pkts > RNS_CHAIN_MAX_PACKETS || n_flows > kFlowMaxFlows)
        return RNS_E_INVALID;
    *bytes = flow_work_bytes(n_pkts, n_flows);
    return RNS_OK;
}
