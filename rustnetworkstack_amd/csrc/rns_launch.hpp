// Host-side launchers of the checksum kernels (rns_kernels.hpp), one translation unit per
// kernel family so the build compiles them in parallel (the declarations below say what each holds):
//   k_shapes.hip, k_packed.hip, k_chain.hip, k_stash.hip  the checksum, fill, verify and finalize forms
//   k_segment.hip, k_place.hip                            TCP segmentation offload, receive placement
//   k_flow.hip, k_conn.hip, k_plan.hip, k_echo.hip,       the sequences of launches; each includes its own kernels
//   k_udp.hip, k_udp_tx.hip, k_listen.hip                 header (rns_k_flow / conn / plan / echo / udp / udp_tx / listen.hpp)
//   (k_place, k_echo and k_udp, the pool verify's consumers, share rns_k_pool_view.hpp: view, decode, walk;
//    k_echo and k_udp_tx, the builders into the pool transmit form, rns_k_pool_txform.hpp and launch_build_seq)
//   k_scan.hip                                            the scan's middle launch, which those seven share
// rns_checksum.hip holds the device entry points of the C ABI, rns_pipeline.hip the host-resident
// pipeline and the multi-GPU contexts.
#pragma once

#include <type_traits>

#include "rns_kernels.hpp"

namespace rns {

inline int hip_status(hipError_t e) { return e == hipSuccess ? RNS_OK : RNS_E_HIP_BASE - static_cast<int>(e); }

// Kernel shape for a typical (mean) packet length, in 16-byte chunks, from the
// interleaved shape sweeps on MI355X (tools/sweep_shapes.py, profiles/r01_sweep*.json):
//   <= 8 chunks   (64 B)        rounds, nontemporal, G=4, U=1, grid 2048,     (c2)
//                               next batch's descriptors prefetched
//   <= 48 chunks  (IMIX mean)   mixed (per-wave size-class sort)              (c5)
//   <= 160 chunks (1500 B)      mixed, nontemporal (= rounds G=32,U=4 here)   (c3, headline)
//   longer        (9000 B)      group, nontemporal, G=64, U=4                 (c4)
// The mixed kernel is the robust choice for any size distribution; the other
// two win by a few percent on batches of uniformly tiny / jumbo packets.
struct Shape {
    uint32_t variant, G, U, max_blocks;
};

// (round 6: the grid caps and the tiny variant are constants, no longer build knobs — every
// shipped shape is one the GPU parity suite runs; the other settings were measured slower:
// a grid cap on the mixed kernel, variant 11 for tiny packets, profiles/archive/r01-r02)
constexpr uint32_t kTinyVariant = 19u;  // rounds, nontemporal, next batch's descriptors prefetched
constexpr uint32_t kTinyGrid = 2048u;   // workgroups (4 waves each) for tiny packets
inline Shape pick_shape(uint32_t len_hint)
{
    const uint32_t chunks = len_hint ? (len_hint + 15) / 16 + 1 : 96;
    if (chunks <= 8)  // rounds, nontemporal, next batch's descriptors prefetched (c2: 15.1 -> 14.4 us)
        return Shape{kTinyVariant, 4u, 1u, kTinyGrid};
    if (chunks <= 48)
        return Shape{4u, 0u, 0u, 0u};  // mixed kernel, one wave per 64-packet batch
    if (chunks <= 160)
        return Shape{6u, 0u, 0u, 0u};
    return Shape{2u, 64u, 4u, 0u};
}

inline int check_device()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return RNS_E_NODEVICE;
    }
    return RNS_OK;
}

// Fill CsumArgs for a caller arena base that may not be 16-byte aligned.
inline void set_arena(CsumArgs &a, const uint8_t *arena, uint64_t arena_bytes)
{
    const uintptr_t p = reinterpret_cast<uintptr_t>(arena);
    a.base_adjust = p & 15;
    a.arena = reinterpret_cast<const uint8_t *>(p - a.base_adjust);
    a.arena_bytes = arena_bytes + a.base_adjust;
}

// Buffer loads need a 32-bit offset range: arenas below 4 GiB take the BUF instantiations.
inline bool buf_ok(const CsumArgs &a) { return buf_records(a) < kOobOffset; }

// Grid of the kernels that give one wave a 64-packet batch.
inline uint32_t waves64(uint64_t n) { return static_cast<uint32_t>((n + 63) / 64); }

// Runtime flags to template arguments: with_flags(f, b0, b1, ...) calls
// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...).  Every combination of the flags
// is instantiated, so a launcher normalises its flags first and cuts the combinations that
// have no kernel with `if constexpr`.
template <class F>
int with_flags(F &&f)
{
    return f();
}
template <class F, class... Rest>
int with_flags(F &&f, bool b, Rest... rest)
{
    auto bind = [&](auto c) { return with_flags([&](auto... cs) { return f(c, cs...); }, rest...); };
    return b ? bind(std::true_type{}) : bind(std::false_type{});
}

// The same for a packets-per-lane bound: with_kmax<1, 2, 8>(K, f) calls f with the first listed
// bound >= K as a std::integral_constant (the last one for any larger K).
template <uint32_t KM, uint32_t... More, class F>
int with_kmax(uint32_t K, F &&f)
{
    if constexpr (sizeof...(More) == 0)
        return f(std::integral_constant<uint32_t, KM>{});
    else
        return K <= KM ? f(std::integral_constant<uint32_t, KM>{}) : with_kmax<More...>(K, f);
}

// One kernel launch and its status.
inline int launch(void (*kernel)(const CsumArgs), dim3 grid, dim3 block, size_t lds, hipStream_t st, const CsumArgs &a)
{
    hipLaunchKernelGGL(kernel, grid, block, lds, st, a);
    return hip_status(hipGetLastError());
}

// One step inside a launcher that is a sequence of them: a status other than RNS_OK is the launcher's.
#define RNS_TRY(status)          \
    do {                         \
        if (int e = (status))    \
            return e;            \
    } while (0)
#define RNS_LAUNCH(kernel, grid, block, st, ...)                                      \
    do {                                                                              \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__);      \
        RNS_TRY(hip_status(hipGetLastError()));                                       \
    } while (0)

// k_scan.hip: the scan's one-workgroup middle launch
int launch_scan2_parts(uint2 *part, uint32_t nb, uint32_t *total2, hipStream_t st);
// k_scan.hip: p[0..n) = v by a kernel: every clear inside a launch sequence (no memset nodes: see the kernel)
int launch_fill32(uint32_t *p, uint64_t n, uint32_t v, hipStream_t st);

// A builder into the pool transmit form (rns_k_pool_txform.hpp) over n items: the counts zeroed, classify(blocks),
// the two scans of its block sums, build(blocks); both return a status.
template <class Classify, class Build>
int launch_build_seq(uint32_t *count, const BuildWork &w, uint64_t n, hipStream_t st, Classify classify, Build build)
{
    const uint32_t nb = static_cast<uint32_t>(scan_blocks(n));
    RNS_TRY(launch_fill32(count, 3, 0u, st));
    RNS_TRY(classify(nb));
    RNS_TRY(launch_scan2_parts(w.part_a, nb, nullptr, st));
    RNS_TRY(launch_scan2_parts(w.part_b, nb, nullptr, st));
    return build(nb);
}

// k_shapes.hip: the explicit-descriptor kernels by (variant, lanes per packet, chunks in flight)
template <bool S>
int dispatch(const CsumArgs &a, uint32_t variant, uint32_t G, uint32_t U, uint32_t max_blocks, hipStream_t st);
extern template int dispatch<false>(const CsumArgs &, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);
extern template int dispatch<true>(const CsumArgs &, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);
int launch_strided_tiny(const CsumArgs &a, hipStream_t st);
// k_packed.hip
int dispatch_packed(const CsumArgs &a, const Shape &sh, hipStream_t st);
int launch_fill_packed(const CsumArgs &a, hipStream_t st);
int launch_stream_rx(const CsumArgs &a, hipStream_t st);
int launch_tx_packed(const CsumArgs &a, hipStream_t st);
int launch_strided_rx(const CsumArgs &a, hipStream_t st);
// k_chain.hip: K packets per lane (1..kChainMaxK); FILL = the head-fragment fill; deep = 4 waves/SIMD
template <bool FILL>
int launch_chain(const CsumArgs &a, uint32_t K, bool nt, bool runs, bool deep, hipStream_t st);
extern template int launch_chain<false>(const CsumArgs &, uint32_t, bool, bool, bool, hipStream_t);
extern template int launch_chain<true>(const CsumArgs &, uint32_t, bool, bool, bool, hipStream_t);
// the transmit-rows kernel: checksum / head-fragment fill (FILL), chain finalize (FIN), compact finalize (FIN, CPT)
template <bool FILL, bool FIN = false, bool CPT = false>
int launch_txrows(const CsumArgs &a, hipStream_t st);
extern template int launch_txrows<false, false, false>(const CsumArgs &, hipStream_t);
extern template int launch_txrows<true, false, false>(const CsumArgs &, hipStream_t);
extern template int launch_txrows<false, true, false>(const CsumArgs &, hipStream_t);
extern template int launch_txrows<false, true, true>(const CsumArgs &, hipStream_t);
int launch_rx_chain(const CsumArgs &a, uint32_t K, bool nt, hipStream_t st);  // receive verify over chains
int launch_rx_pool(const CsumArgs &a, uint32_t K, bool nt, hipStream_t st);   // ... over pool buffers (compact descriptors)
int launch_tx_pool(const CsumArgs &a, uint32_t K, bool nt, hipStream_t st);   // transmit finalize over pool buffers
// k_segment.hip: TCP segmentation offload, one wave per 64 segments
int launch_tx_segment(const CsumArgs &a, bool nt, hipStream_t st);
// k_place.hip: TCP receive placement, one wave per 64-datagram block (after launch_rx_pool on the same stream)
int launch_rx_place(const PlaceArgs &a, bool nt, hipStream_t st);
// k_flow.hip: TCP flow update (count, scan, scatter, walk) and ACK build (scan, build), each a sequence of launches
int launch_flow_update(const FlowArgs &a, hipStream_t st);
int launch_ack_build(const AckArgs &a, hipStream_t st);
int launch_flow_lists(const FlowArgs &a, uint32_t rec_dw, hipStream_t st);  // every flow's datagrams listed (rec_dw: d_seg's 2, d_ctl's 4)
// k_conn.hip: TCP connection update (the flow update's lists, its own walks), control-segment build (scan, build), close step
int launch_conn_update(const FlowArgs &a, hipStream_t st);
int launch_ctl_build(const CtlArgs &a, hipStream_t st);
int launch_conn_close(const CloseArgs &a, hipStream_t st);
// k_plan.hip: TCP send planning (plan, scan, cap, finish), a sequence of launches
int launch_tx_plan(const PlanArgs &a, hipStream_t st);
// k_echo.hip: the ICMP echo responder (classify, two scans, build), after launch_rx_pool on the same stream
int launch_rx_echo(const EchoArgs &a, bool nt, hipStream_t st);
// k_udp.hip: the UDP receive demux (classify, the scan's three, scatter + copy), after launch_rx_pool on the same stream
int launch_rx_udp(const UdpArgs &a, bool nt, hipStream_t st);
// k_udp_tx.hip: the UDP send build (classify, two scans, build)
int launch_tx_udp(const UdpTxArgs &a, hipStream_t st);
// k_listen.hip: the TCP listen responder (clear, classify + insert, resolve, two scans, build), after the placement
int launch_rx_listen(const ListenArgs &a, hipStream_t st);
// k_stash.hip: the class kernel's stash modes on one-wave workgroups
int launch_fill(const CsumArgs &a, dim3 grid, hipStream_t st);
int launch_rx(const CsumArgs &a, dim3 grid, hipStream_t st);
int launch_tx(const CsumArgs &a, dim3 grid, hipStream_t st);

}  // namespace rns
