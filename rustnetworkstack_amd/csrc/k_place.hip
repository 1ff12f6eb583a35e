// TCP receive placement over pool buffers (rns_rx_tcp_place_pool_dev): the decode / lookup / copy
// kernel's launch, one wave per 64-datagram block, and the flow table's host-side builder.
#include <cstring>

#include "rns_launch.hpp"

namespace rns {

int launch_rx_place(const PlaceArgs &a, bool nt, hipStream_t st)
{
    return with_flags(
        [&](auto NT) {
            hipLaunchKernelGGL(rx_place_kernel<NT()>, dim3(waves64(a.n)), dim3(64), 0, st, a);
            return hip_status(hipGetLastError());
        },
        nt);
}

}  // namespace rns

using namespace rns;

extern "C" int rns_rx_flow_table_build(const rns_rx_flow_key *keys, uint32_t n_flows, uint8_t *tbl, uint64_t tbl_bytes,
                                       uint64_t *need_bytes)
{
    if (!need_bytes)
        return RNS_E_INVALID;
    const uint64_t slots = flow_slots(n_flows), need = slots * kFlowSlotBytes;
    *need_bytes = need;
    if (!tbl)
        return RNS_OK;
    if (tbl_bytes < need || (n_flows && !keys))
        return RNS_E_INVALID;
    static_assert(sizeof(rns_rx_flow_key) == 24, "the key is six dwords");
    std::memset(tbl, 0, need);
    for (uint32_t f = 0; f < n_flows; ++f) {
        const rns_rx_flow_key &key = keys[f];
        bool ok = (key.family == 4 || key.family == 6) && !key.pad[0] && !key.pad[1] && !key.pad[2];
        for (int b = 4; ok && key.family == 4 && b < 16; ++b)
            ok = key.ip[b] == 0;
        if (!ok)
            return RNS_E_INVALID;
        uint32_t k[6];
        std::memcpy(k, key.ip, 16);
        k[4] = static_cast<uint32_t>(key.sport) | (static_cast<uint32_t>(key.dport) << 16);
        k[5] = key.family;
        uint64_t s = flow_hash(k) & (slots - 1);
        for (;; s = (s + 1) & (slots - 1)) {  // at most n_flows <= slots / 2 slots are taken: an empty one comes
            uint32_t e[kFlowSlotWords];
            std::memcpy(e, tbl + s * kFlowSlotBytes, kFlowSlotBytes);
            if (e[7] == 0)
                break;
            if (std::memcmp(e, k, sizeof(k)) == 0)
                return RNS_E_INVALID;  // a duplicate key
        }
        const uint32_t e[kFlowSlotWords] = {k[0], k[1], k[2], k[3], k[4], k[5], f, 1u};
        std::memcpy(tbl + s * kFlowSlotBytes, e, kFlowSlotBytes);
    }
    return RNS_OK;
}
