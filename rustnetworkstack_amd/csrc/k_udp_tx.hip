// UDP send build (rns_tx_udp_send_pool_dev): the launch sequence — every grid-wide dependency is a launch
// boundary on the one stream — and the workspace's host-side sizing.
#include "rns_launch.hpp"
#include "rns_k_udp_tx.hpp"

namespace rns {

int launch_tx_udp(const UdpTxArgs &a, hipStream_t st)
{
    return launch_build_seq(
        a.tx.count, a.w, a.n_recs, st,
        [&](uint32_t nb) {
            RNS_LAUNCH(udp_tx_classify_kernel, nb, kScanBlock, st, a);
            return static_cast<int>(RNS_OK);
        },
        [&](uint32_t nb) {
            RNS_LAUNCH(udp_tx_build_kernel, nb, kScanBlock, st, a);
            return static_cast<int>(RNS_OK);
        });
}

}  // namespace rns

using namespace rns;

extern "C" int rns_tx_udp_send_work(uint32_t n_recs, uint64_t *bytes)
{
    if (!bytes || n_recs > RNS_CHAIN_MAX_PACKETS)
        return RNS_E_INVALID;
    *bytes = udp_tx_work_bytes(n_recs);
    return RNS_OK;
}
