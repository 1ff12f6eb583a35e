// TCP connection update, control-segment build and close step (rns_rx_tcp_conn_update_dev,
// rns_tx_tcp_ctl_build_dev, rns_tx_tcp_close_dev): the launch sequences and the workspaces' host-side sizing.
// The update's lists are the flow update's launches (launch_flow_lists, k_flow.hip).
#include "rns_launch.hpp"
#include "rns_k_conn.hpp"

namespace rns {

static uint32_t blocks_of(uint64_t n) { return static_cast<uint32_t>(scan_blocks(n)); }

int launch_conn_update(const FlowArgs &a, hipStream_t st)
{
    RNS_TRY(launch_flow_lists(a, ConnStepOp::kRecDw, st));
    if (a.n_flows == 0)
        return RNS_OK;
    RNS_LAUNCH(conn_walk_lane_kernel, blocks_of(a.n_flows), kScanBlock, st, a);
    if (a.n_pkts >= 2)  // a flow with two datagrams exists only then, and at most n_pkts / 2 of them
        RNS_LAUNCH(conn_walk_wave_kernel, std::min({a.n_flows, a.n_pkts / 2, kFlowWaveGrid}), 64, st, a);
    return RNS_OK;
}

int launch_ctl_build(const CtlArgs &a, hipStream_t st)
{
    if (a.n_ctl == 0)
        return launch_fill32(a.count, 2, 0u, st);
    const uint32_t nb = blocks_of(a.n_ctl);
    RNS_LAUNCH((scan2_reduce_kernel<CtlValue, CtlArgs>), nb, kScanBlock, st, a, static_cast<uint64_t>(a.n_ctl), a.part);
    RNS_TRY(launch_scan2_parts(a.part, nb, a.count, st));
    if (a.out_cap)
        RNS_LAUNCH(ctl_build_kernel, nb, kScanBlock, st, a);
    return RNS_OK;
}

int launch_conn_close(const CloseArgs &a, hipStream_t st)
{
    RNS_LAUNCH(conn_close_kernel, blocks_of(a.n_flows), kScanBlock, st, a);
    return RNS_OK;
}

}  // namespace rns

using namespace rns;

extern "C" int rns_rx_tcp_conn_update_work(uint32_t n_pkts, uint32_t n_flows, uint64_t *bytes)
{
    if (!bytes || n_pkts > RNS_CHAIN_MAX_PACKETS || n_flows > kFlowMaxFlows)
        return RNS_E_INVALID;
    *bytes = flow_work_bytes(n_pkts, n_flows);
    return RNS_OK;
}

extern "C" int rns_tx_tcp_ctl_build_work(uint32_t n_ctl, uint64_t *bytes)
{
    if (!bytes || n_ctl > RNS_CHAIN_MAX_PACKETS)
        return RNS_E_INVALID;
    *bytes = ctl_work_bytes(n_ctl);
    return RNS_OK;
}
