// The packed form (rns_csum_batch_packed_dev) and packed receive verify.
#include "rns_launch.hpp"

#ifndef RNS_ROWS_DEEP_FROM  // typical lengths from this take D = 16 rows in flight at 4 waves/SIMD
#define RNS_ROWS_DEEP_FROM 1024u
#endif
#ifndef RNS_TX_ROWS_DEEP_FROM  // typical lengths from this take D = 16 rows at 4 waves/SIMD
#define RNS_TX_ROWS_DEEP_FROM 1024u
#endif
#ifndef RNS_RX_ROWS_D  // rows in flight of the receive form
#define RNS_RX_ROWS_D 8
#endif

namespace rns {

constexpr bool kStreamNT = RNS_STREAM_NT != 0;

// The rows kernels' launch, one wave per 64 packets: D = 16 rows in flight for typical lengths
// from `deep_from`, else 8, on the buffer path where the arena allows it.  `kernel(D, buf)`
// names the instantiation.
template <class Kernel>
static int launch_rows(const CsumArgs &a, uint32_t deep_from, hipStream_t st, Kernel kernel)
{
    return with_flags(
        [&](auto deep, auto buf) {
            return launch(kernel(std::integral_constant<int, deep() ? 16 : 8>{}, buf), dim3(waves64(a.n)), dim3(64), 0,
                          st, a);
        },
        a.len_hint >= deep_from, buf_ok(a));
}

// The packed form's kernels (separate instantiations, so the explicit-descriptor
// kernels carry no packed-form code): the mixed kernel, or for tiny packets the
// rounds kernel with pick_shape's G=4, U=1 shape.
// Receive verify's stream launch: one wave per 64-datagram unit.
// Packed receive verify: the rows receive kernel (round 5: IMIX 468.1 -> 449.2-450.3 us, c3
// 230.4 -> 225.0-226.2 per step against the stream kernel), except for arenas of ACK-sized
// datagrams (at most 128 arena bytes per datagram), where the stream kernel's ACK path measured
// faster (14.54-14.64 vs 15.03-15.25 us per isolated dispatch; sessions r05c-r05h; a kernel of
// its own, 1 or 2 units per wave at 6-8 waves/SIMD: 15.2-19.5 against 14.7-14.9, r05n).
int launch_stream_rx(const CsumArgs &a, hipStream_t st)
{
    return with_flags(
        [&](auto ack, auto buf) {
            if constexpr (ack())
                return launch(csum_stream_kernel<kStreamNT, buf()>, dim3(waves64(a.n)), dim3(64), 0, st, a);
            else
                return launch(csum_rows_rx_kernel<kStreamNT, buf(), RNS_RX_ROWS_D>, dim3(waves64(a.n)), dim3(64), 0, st,
                              a);
        },
        a.arena_bytes / a.n <= 128, buf_ok(a));
}

int dispatch_packed(const CsumArgs &a, const Shape &sh, hipStream_t st)
{
    // 16-byte-aligned packets (align_log2 >= 4) of any typical length above the tiny rounds
    // kernel's, or unknown: the rows kernel.  Measured against the kernels it replaced (session
    // r04d, isolated dispatch): c3 1500 B 231.5 vs 238.5-239.2 us (class kernel), c4 9000 B
    // 344.4-345.1 vs 346.4-347.1 (group kernel, u32 offsets), IMIX 451-453 vs 456 (round 3's
    // stream kernel).  Tiny packets keep the rounds kernel (c2: 13.2-13.7 vs 14.0-14.8 us with
    // round 3's stream kernel).
    // (tiny packets through the rows kernel: c2 19.6 vs 13.8 us per isolated dispatch, a 4 KiB unit
    // is all prologue: profiles/r04_unit_size_and_tiny.json)
    const bool tiny = (sh.variant & ~16u) == 3u && sh.G == 4u && sh.U == 1u;
    if (a.align_mask >= 15u && !tiny)
        return launch_rows(a, RNS_ROWS_DEEP_FROM, st,
                           [](auto D, auto buf) { return csum_rows_kernel<kStreamNT, buf(), D()>; });
    const bool mixed = (sh.variant & 4u) != 0;
    if (!mixed && !tiny)
        return RNS_E_INVALID;
    const uint64_t batches = waves64(a.n);  // one wave per 64 packets
    const uint64_t wpb = (mixed ? kMixedBlock<false> : kBlock) / 64;  // waves per workgroup
    uint64_t blocks = (batches + wpb - 1) / wpb;
    if (sh.max_blocks != 0 && blocks > sh.max_blocks)
        blocks = sh.max_blocks;
    const dim3 grid(static_cast<uint32_t>(blocks)), block(mixed ? kMixedBlock<false> : kBlock);
    if (mixed)
        return with_flags(
            [&](auto nt, auto buf) {
                return launch(csum_mixed_kernel<false, nt(), buf(), false, false, false, true>, grid, block, 0, st, a);
            },
            (sh.variant & 2u) != 0, buf_ok(a));
    return with_flags(  // c2: 13.46 -> 13.36 us with prefetch
        [&](auto buf, auto pf) {
            return launch(csum_rounds_kernel<4, 1, false, true, buf(), 1, true, pf()>, grid, block, 0, st, a);
        },
        buf_ok(a), (sh.variant & 16u) != 0);
}

// Transmit fill of a packed arena (align_log2 >= 4): the rows kernel in fill mode, D by the
// typical length as for the plain checksum.
// (Temporal row loads, so that a field's line is still in L2 when its store comes, measured
// slower on c3 and equal on IMIX: fill 344.4 / 762.3 us, finalize 360.8 / 808.8 against
// 303.8 / 764.2 and 306.7 / 810.9 with nontemporal rows; session r06d.)
int launch_fill_packed(const CsumArgs &a, hipStream_t st)
{
    return launch_rows(a, RNS_ROWS_DEEP_FROM, st,
                       [](auto D, auto buf) { return csum_rows_kernel<kStreamNT, buf(), D(), true>; });
}

// Transmit finalize of a packed arena (align_log2 >= 4): the rows transmit kernel, D by the
// typical length as for the plain checksum.
int launch_tx_packed(const CsumArgs &a, hipStream_t st)
{
    return launch_rows(a, RNS_TX_ROWS_DEEP_FROM, st,
                       [](auto D, auto buf) { return csum_rows_tx_kernel<kStreamNT, buf(), D()>; });
}

// Receive verify of datagrams at a fixed stride: B batches of 64 per one-wave workgroup (one:
// 48 VGPRs, 10 waves/SIMD; two batches per wave need 81 VGPRs and a second generation of waves,
// 16.4 us per isolated 64-byte dispatch against 14.0: sessions r06c, r06d).
int launch_strided_rx(const CsumArgs &a, hipStream_t st)
{
    constexpr int B = kStridedRxB;
    const dim3 grid(static_cast<uint32_t>((static_cast<uint64_t>(a.n) + 64 * B - 1) / (64 * B)));
    return with_flags([&](auto buf) { return launch(csum_strided_rx_kernel<buf(), B>, grid, dim3(64), 0, st, a); },
                      buf_ok(a));
}

}  // namespace rns
