// TCP listen responder (rns_rx_tcp_listen_pool_dev): the launch sequence after the placement — every
// grid-wide dependency is a launch boundary on the one stream — and the workspace's host-side sizing.
#include "rns_launch.hpp"
#include "rns_k_listen.hpp"

namespace rns {

int launch_rx_listen(const ListenArgs &a, hipStream_t st)
{
    const uint32_t nb = static_cast<uint32_t>(scan_blocks(a.rx.n));
    // every slot kListenEmpty64, kListenEmpty: tbl's 8 and first's 4 bytes per slot lie one after the other
    RNS_TRY(launch_fill32(reinterpret_cast<uint32_t *>(a.tbl), 3ull * a.slots, kListenEmpty, st));
    RNS_LAUNCH(listen_classify_kernel, nb, kScanBlock, st, a);
    RNS_LAUNCH(listen_resolve_kernel, nb, kScanBlock, st, a);
    RNS_TRY(launch_scan2_parts(a.w.part_a, nb, nullptr, st));
    RNS_TRY(launch_scan2_parts(a.w.part_b, nb, nullptr, st));
    RNS_LAUNCH(listen_build_kernel, nb, kScanBlock, st, a);
    return RNS_OK;
}

}  // namespace rns

using namespace rns;

extern "C" int rns_rx_tcp_listen_work(uint32_t n_pkts, uint64_t *bytes)
{
    if (!bytes || n_pkts > RNS_CHAIN_MAX_PACKETS)
        return RNS_E_INVALID;
    *bytes = listen_work_bytes(n_pkts);
    return RNS_OK;
}
