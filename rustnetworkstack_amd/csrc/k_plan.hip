// TCP send planning (rns_tx_tcp_plan_dev): the launch sequence — every grid-wide dependency is a
// launch boundary on the one stream — and the workspace's host-side sizing.
#include "rns_launch.hpp"
#include "rns_k_plan.hpp"

namespace rns {

int launch_tx_plan(const PlanArgs &a, hipStream_t st)
{
    if (a.n_flows == 0) {  // no entry: E = 0 names every block, and the totals are zero
        RNS_TRY(launch_fill32(a.seg_first, 1, 0u, st));
        RNS_TRY(launch_fill32(a.n_out, 2, 0u, st));
        return launch_fill32(a.blk_flow, (static_cast<uint64_t>(a.seg_cap) + 63) / 64, 0u, st);
    }
    const uint64_t E = 2ull * a.n_flows;
    const uint32_t nf = static_cast<uint32_t>(scan_blocks(a.n_flows)), nb = static_cast<uint32_t>(scan_blocks(E));
    RNS_LAUNCH(plan_flow_kernel, nf, kScanBlock, st, a);
    RNS_LAUNCH((scan2_reduce_kernel<PlanValue, PlanArgs>), nb, kScanBlock, st, a, E, a.part);
    RNS_TRY(launch_scan2_parts(a.part, nb, nullptr, st));
    RNS_LAUNCH(plan_cap_kernel, 1, kScanBlock, st, a);
    RNS_LAUNCH(plan_finish_kernel, nf, kScanBlock, st, a);
    return RNS_OK;
}

}  // namespace rns

using namespace rns;

extern "C" int rns_tx_tcp_plan_work(uint32_t n_flows, uint64_t *bytes)
{
    if (!bytes || n_flows > kPlanMaxFlows)
        return RNS_E_INVALID;
    *bytes = plan_work_bytes(n_flows);
    return RNS_OK;
}
