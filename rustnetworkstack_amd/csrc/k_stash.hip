// The class kernel's stash modes on one-wave workgroups: transmit fill (rns_csum_fill_dev),
// receive verify (rns_rx_verify_dev) and transmit finalize (rns_tx_fill_dev).
#include "rns_launch.hpp"

namespace rns {

// FILL / RX / TX: the mode's flag of csum_mixed_kernel; NT: nontemporal loads.
template <bool NT, bool FILL, bool RX, bool TX>
static int launch_stash(const CsumArgs &a, dim3 grid, hipStream_t st)
{
    return with_flags(
        [&](auto buf) {
            return launch(csum_mixed_kernel<false, NT, buf(), FILL, RX, TX>, grid, dim3(kMixedBlock<true>), 0, st, a);
        },
        buf_ok(a));
}

int launch_fill(const CsumArgs &a, dim3 grid, hipStream_t st) { return launch_stash<false, true, false, false>(a, grid, st); }

// nontemporal loads
int launch_rx(const CsumArgs &a, dim3 grid, hipStream_t st) { return launch_stash<true, false, true, false>(a, grid, st); }

int launch_tx(const CsumArgs &a, dim3 grid, hipStream_t st) { return launch_stash<false, false, false, true>(a, grid, st); }

}  // namespace rns
