// The scan's one-workgroup middle launch (rns_k_scan.hpp): the one kernel of the scan that is no
// template, and its launcher; and the fill a launch sequence clears a table with.
#include "rns_launch.hpp"

namespace rns {

// part[0..nb) to its exclusive prefix sums, part[nb] = the total (and *total2, when given): one workgroup
__global__ __launch_bounds__(kScanBlock) void scan2_parts_kernel(uint2 *part, uint32_t nb, uint32_t *total2)
{
    uint2 carry = make_uint2(0u, 0u);
    for (uint32_t base = 0; base < nb; base += kScanBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint2 v = i < nb ? part[i] : make_uint2(0u, 0u);
        uint2 total;
        const uint2 ex = scan2_block(v, total);
        if (i < nb)
            part[i] = make_uint2(carry.x + ex.x, carry.y + ex.y);
        carry.x += total.x;
        carry.y += total.y;
    }
    if (threadIdx.x == 0) {
        part[nb] = carry;
        if (total2) {
            total2[0] = carry.x;
            total2[1] = carry.y;
        }
    }
}

int launch_scan2_parts(uint2 *part, uint32_t nb, uint32_t *total2, hipStream_t st)
{
    RNS_LAUNCH(scan2_parts_kernel, 1, kScanBlock, st, part, nb, total2);
    return RNS_OK;
}

// p[0..n) = v.  What a launch sequence zeroes or clears before its first kernel it clears with this kernel and not
// with hipMemsetAsync: captured into a graph, a memset node wrote its pattern on the first replay and other bytes
// on later ones (tests/test_gpu_streams.py found the listen responder's table and the flow lists' counts so).
__global__ __launch_bounds__(kScanBlock) void fill32_kernel(uint32_t *p, uint64_t n, uint32_t v)
{
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x; i < n;
         i += static_cast<uint64_t>(gridDim.x) * kScanBlock)
        p[i] = v;
}

int launch_fill32(uint32_t *p, uint64_t n, uint32_t v, hipStream_t st)
{
    if (n == 0)
        return RNS_OK;
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((n + kScanBlock - 1) / kScanBlock, 4096));
    RNS_LAUNCH(fill32_kernel, grid, kScanBlock, st, p, n, v);
    return RNS_OK;
}

}  // namespace rns
