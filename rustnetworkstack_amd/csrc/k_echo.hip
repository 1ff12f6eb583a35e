// ICMP echo responder (rns_rx_icmp_echo_pool_dev): the launch sequence after the pool verify — every
// grid-wide dependency is a launch boundary on the one stream — and the workspace's host-side sizing.
#include "rns_launch.hpp"
#include "rns_k_echo.hpp"

namespace rns {

int launch_rx_echo(const EchoArgs &a, bool nt, hipStream_t st)
{
    return launch_build_seq(
        a.tx.count, a.w, a.rx.n, st,
        [&](uint32_t nb) {
            RNS_LAUNCH(echo_classify_kernel, nb, kScanBlock, st, a);
            return static_cast<int>(RNS_OK);
        },
        [&](uint32_t nb) {
            return with_flags(
                [&](auto NT) {
                    RNS_LAUNCH(echo_build_kernel<NT()>, nb, kScanBlock, st, a);
                    return static_cast<int>(RNS_OK);
                },
                nt);
        });
}

}  // namespace rns

using namespace rns;

extern "C" int rns_rx_icmp_echo_work(uint32_t n_pkts, uint64_t *bytes)
{
    if (!bytes || n_pkts > RNS_CHAIN_MAX_PACKETS)
        return RNS_E_INVALID;
    *bytes = echo_work_bytes(n_pkts);
    return RNS_OK;
}
