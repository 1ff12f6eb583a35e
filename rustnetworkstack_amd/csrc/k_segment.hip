// TCP segmentation offload (rns_tx_segment_dev): one wave per 64 segments.
#include "rns_launch.hpp"

namespace rns {

int launch_tx_segment(const CsumArgs &a, bool nt, hipStream_t st)
{
    return with_flags([&](auto NT, auto BUF) { return launch(tx_segment_kernel<NT(), BUF()>, dim3(waves64(a.n)), dim3(64), 0, st, a); },
                      nt, buf_ok(a));
}

}  // namespace rns
