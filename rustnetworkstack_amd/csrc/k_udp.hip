// UDP receive demux (rns_rx_udp_demux_pool_dev): the launch sequence after the pool verify — every
// grid-wide dependency is a launch boundary on the one stream — the workspace's host-side sizing and the
// port table's host-side builder.
#include "rns_launch.hpp"
#include "rns_k_udp.hpp"

namespace rns {

int launch_rx_udp(const UdpArgs &a, bool nt, hipStream_t st)
{
    const uint64_t m = static_cast<uint64_t>(a.n_socks) * a.n_tiles;
    const uint32_t nb = static_cast<uint32_t>(scan_blocks(m));
    RNS_LAUNCH(udp_classify_kernel, a.n_tiles, kScanBlock, st, a);
    if (m) {
        RNS_LAUNCH((scan2_reduce_kernel<UdpMatValue, UdpArgs>), nb, kScanBlock, st, a, m, a.part);
        RNS_TRY(launch_scan2_parts(a.part, nb, a.count, st));
        RNS_LAUNCH(udp_prefix_kernel, nb, kScanBlock, st, a, m);
    } else {  // no socket: no entry
        RNS_TRY(launch_fill32(a.count, 2, 0u, st));
        RNS_TRY(launch_fill32(a.q_first, 1, 0u, st));
    }
    return with_flags(
        [&](auto NT) {
            RNS_LAUNCH(udp_scatter_kernel<NT()>, a.n_tiles, kScanBlock, st, a);
            return static_cast<int>(RNS_OK);
        },
        nt);
}

}  // namespace rns

using namespace rns;

extern "C" int rns_rx_udp_demux_work(uint32_t n_pkts, uint32_t n_socks, uint64_t *bytes)
{
    if (!bytes || n_pkts > RNS_CHAIN_MAX_PACKETS || n_socks > RNS_UDP_MAX_SOCKS)
        return RNS_E_INVALID;
    *bytes = udp_work_bytes(n_pkts, n_socks);
    return RNS_OK;
}

extern "C" int rns_rx_udp_port_table_build(const uint16_t *ports, uint32_t n_socks, uint16_t *tbl)
{
    if (!tbl || n_socks > RNS_UDP_MAX_SOCKS || (n_socks && !ports))
        return RNS_E_INVALID;
    for (uint32_t p = 0; p < 65536u; ++p)
        tbl[p] = RNS_UDP_NO_SOCK;
    for (uint32_t s = 0; s < n_socks; ++s) {
        if (tbl[ports[s]] != RNS_UDP_NO_SOCK)
            return RNS_E_INVALID;  // udp_open: "Port already in use"
        tbl[ports[s]] = static_cast<uint16_t>(s);
    }
    return RNS_OK;
}
