// The grid-wide exclusive prefix sum of pairs of u32, 256 per workgroup, in three launches on one
// stream, for the flow update, the ACK build, the send planning, the echo responder, the UDP demux and the
// UDP send build:
//   1. scan2_reduce_kernel<V, A>: part[b] = block b's sum of V::value(a, i) (or the user's own kernel).
//   2. scan2_parts_kernel, one workgroup: part[0..nb) to its exclusive prefix sums, part[nb] = the total.
//      It is no template, so k_scan.hip alone compiles it, with its launcher launch_scan2_parts.
//   3. the user's consumer kernel scans its block again with scan2_block and adds part[block].
// (One part of rns_kernels.hpp: the parts are included in order, each after the one it builds on.)
#pragma once

#include "rns_k_tcp_head.hpp"

namespace rns {

// (plain C++ that a host compiler takes: the workspace formulas are written over it)
constexpr uint32_t kScanBlock = 256;
RNS_HD uint64_t scan_blocks(uint64_t n) { return (n + kScanBlock - 1) / kScanBlock; }

}  // namespace rns

#ifdef __HIPCC__
#include "rns_k_common.hpp"

namespace rns {

__device__ __forceinline__ uint2 scan2_block(uint2 v, uint2 &total)
{
    __shared__ uint2 ws[kScanBlock / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint2 inc = make_uint2(wave_incl_scan(v.x), wave_incl_scan(v.y));
    __syncthreads();  // a call before this one has read ws
    if (lane == 63)
        ws[w] = inc;
    __syncthreads();
    uint2 before = make_uint2(0u, 0u);
    total = make_uint2(0u, 0u);
#pragma unroll
    for (uint32_t k = 0; k < kScanBlock / 64; ++k) {
        const uint2 s = ws[k];
        if (k < w) {
            before.x += s.x;
            before.y += s.y;
        }
        total.x += s.x;
        total.y += s.y;
    }
    return make_uint2(before.x + inc.x - v.x, before.y + inc.y - v.y);
}

// part[b] = the sum of block b's values
template <class V, class A>
__global__ __launch_bounds__(kScanBlock) void scan2_reduce_kernel(const A a, uint64_t n, uint2 *part)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    const uint2 v = i < n ? V::value(a, i) : make_uint2(0u, 0u);
    uint2 total;
    (void)scan2_block(v, total);
    if (threadIdx.x == 0)
        part[blockIdx.x] = total;
}

}  // namespace rns
#endif  // __HIPCC__
