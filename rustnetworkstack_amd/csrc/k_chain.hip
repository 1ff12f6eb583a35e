// Fragment chains (rns_csum_chain_dev) and their head-fragment fill (rns_csum_chain_fill_dev):
// the one-pass class kernel, K packets per lane; its receive forms over CSR chains and pool buffers and
// the transmit finalize over pool buffers.
#include "rns_launch.hpp"

namespace rns {

// The kernel set: the run-checking form exists on the buffer path only, and the form at
// 4 waves/SIMD (`deep`, the caller's choice by the chain shape) only for the temporal plain
// checksum on the buffer path without the run check.  The flags are normalised to that set.
template <bool FILL>
int launch_chain(const CsumArgs &a, uint32_t K, bool nt, bool runs, bool deep, hipStream_t st)
{
    const uint64_t waves = (static_cast<uint64_t>(a.n) + 64 * K - 1) / (64 * K);
    const dim3 grid(static_cast<uint32_t>((waves + kChainBlock / 64 - 1) / (kChainBlock / 64))), block(kChainBlock);
    const bool buf = buf_ok(a);
    runs = runs && buf;
    deep = deep && !FILL && !nt && buf && !runs;
    return with_kmax<1, kChainMaxK>(K, [&](auto KM) {
        return with_flags(
            [&](auto NT, auto BUF, auto RUNS, auto DEEP) {
                if constexpr ((RUNS() && !BUF()) || (DEEP() && (FILL || NT() || !BUF() || RUNS())))
                    return static_cast<int>(RNS_E_INVALID);  // not in the kernel set, and normalised away above
                else
                    return launch(csum_chain_kernel<NT(), BUF(), KM(), RUNS(), FILL, DEEP() ? 4 : 0>, grid, block, 0, st,
                                  a);
            },
            nt, buf, runs, deep);
    });
}

// The transmit-rows kernel (one wave per 64 packets), by its mode:
//   <FILL>              RNS_FLAG_CHAIN_TX_PACKED: the checksum (false) or head-fragment fill (true) of
//                       transmit-shaped chains;
//   <false, FIN>        transmit finalize of chains (rns_tx_fill_chain_dev), whatever the batch's shape
//                       (a wave without the transmit-packed shape takes its exact per-packet loop);
//   <false, FIN, CPT>   the same finalize over the compact descriptors (rns_tx_fill_chain_packed_dev).
#ifndef RNS_TXROWS_D  // payload rows in flight per wave
#define RNS_TXROWS_D 8
#endif
template <bool FILL, bool FIN, bool CPT>
int launch_txrows(const CsumArgs &a, hipStream_t st)
{
    return with_flags(
        [&](auto buf) {
            return launch(csum_txrows_kernel<RNS_STREAM_NT != 0, buf(), RNS_TXROWS_D, FILL, FIN, CPT>, dim3(waves64(a.n)),
                          dim3(64), 0, st, a);
        },
        buf_ok(a));
}

// Receive verify over chains (rns_rx_verify_chain_dev): the chain kernel's receive form, one wave per
// K*64 datagrams.
int launch_rx_chain(const CsumArgs &a, uint32_t K, bool nt, hipStream_t st)
{
    const uint64_t waves = (static_cast<uint64_t>(a.n) + 64 * K - 1) / (64 * K);
    const dim3 grid(static_cast<uint32_t>(waves)), block(kChainBlock);
    return with_kmax<1, 2, kChainMaxK>(K, [&](auto KM) {
        return with_flags([&](auto NT, auto BUF) { return launch(rx_chain_kernel<NT(), BUF(), KM()>, grid, block, 0, st, a); },
                          nt, buf_ok(a));
    });
}

// Receive verify over pool buffers (rns_rx_verify_pool_dev): one wave per K*64 datagrams, one batch each.
int launch_rx_pool(const CsumArgs &a, uint32_t K, bool nt, hipStream_t st)
{
    const uint64_t waves = (static_cast<uint64_t>(a.n) + 64 * K - 1) / (64 * K);
    const dim3 grid(static_cast<uint32_t>(waves)), block(kChainBlock);
    return with_kmax<1, 2, kChainMaxK>(K, [&](auto KM) {
        return with_flags([&](auto NT, auto BUF) { return launch(rx_pool_kernel<NT(), BUF(), KM()>, grid, block, 0, st, a); },
                          nt, buf_ok(a));
    });
}

// Transmit finalize over pool buffers (rns_tx_fill_pool_dev): one wave per K*64 datagrams, one batch each.
int launch_tx_pool(const CsumArgs &a, uint32_t K, bool nt, hipStream_t st)
{
    const uint64_t waves = (static_cast<uint64_t>(a.n) + 64 * K - 1) / (64 * K);
    const dim3 grid(static_cast<uint32_t>(waves)), block(kChainBlock);
    return with_kmax<1, 2, kChainMaxK>(K, [&](auto KM) {
        return with_flags([&](auto NT, auto BUF) { return launch(tx_pool_kernel<NT(), BUF(), KM()>, grid, block, 0, st, a); },
                          nt, buf_ok(a));
    });
}

template int launch_chain<false>(const CsumArgs &, uint32_t, bool, bool, bool, hipStream_t);
template int launch_chain<true>(const CsumArgs &, uint32_t, bool, bool, bool, hipStream_t);
template int launch_txrows<false, false, false>(const CsumArgs &, hipStream_t);
template int launch_txrows<true, false, false>(const CsumArgs &, hipStream_t);
template int launch_txrows<false, true, false>(const CsumArgs &, hipStream_t);
template int launch_txrows<false, true, true>(const CsumArgs &, hipStream_t);

}  // namespace rns
