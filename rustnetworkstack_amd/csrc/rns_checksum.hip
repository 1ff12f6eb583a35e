// The device entry points of the C ABI (include/rns_checksum.h): argument checks and the batch
// descriptors -> CsumArgs.  The kernels are in rns_kernels.hpp and are launched from the k_*.hip
// translation units (rns_launch.hpp); the host-resident pipeline and the multi-GPU contexts are
// in rns_pipeline.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "rns_launch.hpp"

using namespace rns;

namespace {

__global__ __launch_bounds__(kBlock) void splitmix64_fill_kernel(uint8_t *buf, uint64_t nbytes, uint64_t seed)
{
    const uint64_t nwords = (nbytes + 7) / 8;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nwords; i += stride) {
        uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        if ((i + 1) * 8 <= nbytes) {
            reinterpret_cast<uint64_t *>(buf)[i] = z;
        } else {
            for (uint64_t b = i * 8; b < nbytes; ++b)
                buf[b] = static_cast<uint8_t>(z >> (8 * (b - i * 8)));
        }
    }
}

// Every device entry point opens the same way, and the order is part of the ABI: an empty batch
// is RNS_OK before any pointer is looked at, an argument error (`valid` false) is RNS_E_INVALID
// before the device is asked for, then RNS_E_NODEVICE.  `body` gets the CsumArgs with the arena,
// n and flags set, fills in its descriptors and launches.
template <class Body>
int entry(uint32_t n, bool valid, const uint8_t *d_arena, uint64_t arena_bytes, uint32_t flags, void *stream, Body body)
{
    if (n == 0)
        return RNS_OK;
    if (!d_arena || !valid)
        return RNS_E_INVALID;
    RNS_TRY(check_device());
    CsumArgs a{};
    set_arena(a, d_arena, arena_bytes);
    a.n = n;
    a.flags = flags;
    return body(a, static_cast<hipStream_t>(stream));
}

// --- descriptor forms ---
void set_explicit(CsumArgs &a, const uint64_t *d_off, const uint32_t *d_len)
{
    a.off = d_off;
    a.len = d_len;
}

// u16 lengths, one offset per 64 packets, starts at 2^align_log2 boundaries (each entry point
// has its own align_log2 range: packed_align)
void set_packed(CsumArgs &a, const uint64_t *d_blk_off, const uint16_t *d_len16, uint32_t align_log2)
{
    a.len16 = d_len16;
    a.blk_off = d_blk_off;
    a.align_mask = (1u << align_log2) - 1u;
}

bool packed_align(uint32_t align_log2, uint32_t lo) { return align_log2 >= lo && align_log2 <= 12; }

void set_strided(CsumArgs &a, uint64_t first_off, uint64_t stride)
{
    a.first_off = first_off;
    a.stride = stride;
}

// A strided call's offsets first_off + i * stride (+ the base adjustment) must not wrap 64 bits:
// a wrapped offset would name bytes inside the arena that are not packet i's.
bool strided_fits(uint64_t first_off, uint64_t stride, uint32_t n)
{
    const uint64_t room = ~0ull - 16u - first_off;
    return first_off <= ~0ull - 16u && (n <= 1 || stride <= room / (n - 1));
}

void set_chain(CsumArgs &a, const uint64_t *d_frag_off, const uint32_t *d_frag_len, const uint32_t *d_first,
               uint32_t n_frags)
{
    a.off = d_frag_off;
    a.len = d_frag_len;
    a.first = d_first;
    a.n_frags = n_frags;
}

// the chain kernels add packet indices in 32 bits (a VGPR less across the class pass): the
// last wave's base + 64 * K + lane must not wrap
static_assert(RNS_CHAIN_MAX_PACKETS == 0xFFFFFFFFu - 64u * kChainMaxK, "rns_checksum.h's chain cap");
bool chain_valid(const uint64_t *d_frag_off, const uint32_t *d_frag_len, const uint32_t *d_first, uint32_t n_frags,
                 uint32_t n_pkts)
{
    return d_first && (!n_frags || (d_frag_off && d_frag_len)) && n_pkts <= RNS_CHAIN_MAX_PACKETS;
}

// --- results and modes ---
void set_results(CsumArgs &a, const uint16_t *d_seed, uint16_t *d_out, uint32_t *d_bad)
{
    a.seed = d_seed;
    a.out = d_out;
    a.bad = d_bad;
}

void set_field(CsumArgs &a, const uint16_t *d_field, uint32_t field_off)
{
    a.field = d_field;
    a.field_off = field_off;
}

uint32_t be_sum(const uint8_t *p, int nbytes)
{
    uint32_t s = 0;
    for (int k = 0; k < nbytes; k += 2)
        s += static_cast<uint32_t>(p[k]) << 8 | p[k + 1];
    return s;
}

// receive verify: the status / L4-sum outputs and the local addresses (non-null: rx_valid)
void set_rx(CsumArgs &a, uint8_t *d_status, uint16_t *d_l4_sum, const uint8_t *local_ipv4, const uint8_t *local_ipv6)
{
    a.status = d_status;
    a.l4_out = d_l4_sum;
    a.local4_sum = be_sum(local_ipv4, 4);
    a.local6_sum = be_sum(local_ipv6, 16);
}

bool rx_valid(const uint8_t *d_status, const uint8_t *local_ipv4, const uint8_t *local_ipv6)
{
    return d_status && local_ipv4 && local_ipv6;
}

void set_tx_status(CsumArgs &a, uint8_t *d_status) { a.status = d_status; }

// --- the chain kernels' decisions ---
// Packets per lane K for a mean fragment count: the wave's K*64 packets should bring whole
// 64-fragment batches (a partial batch runs the class rounds for few bytes), so pick the K
// in 1..8 whose expected fragment count K*mean fills its batches best.
uint32_t chain_pick_k(double mean)
{
    uint32_t K = 1;
    double best = -1.0;
    for (uint32_t k = 1; k <= kChainMaxK; ++k) {
        const double fr = k * mean, fill = fr > 0 ? fr / std::ceil(fr) : 1.0;
        if (fill > best + 0.02) {
            best = fill;
            K = k;
        }
    }
    return K;
}

double chain_mean(const CsumArgs &a) { return static_cast<double>(a.n_frags) / static_cast<double>(a.n); }

// Nontemporal loads for NetBuffer-sized fragments (c3 as 3 fragments: 298 -> 289 us
// packed back to back, 281 -> 261 us in 512-byte buffers), not for IMIX's mix of
// 40-byte packets and 512-byte fragments (646 -> 670 us): profiles/archive/r02/r02_chain_ab.json.
#ifndef RNS_CHAIN_NT_FROM  // fragment lengths from this take the nontemporal instantiation
#define RNS_CHAIN_NT_FROM 384u
#endif
// ... from the caller's fragment-length hint (checksum, fill),
bool chain_nt_from_hint(uint32_t frag_len_hint) { return (frag_len_hint ? frag_len_hint : 512u) >= RNS_CHAIN_NT_FROM; }
// ... or, where no hint travels (receive verify), from an estimate of the typical fragment
// length: the arena's bytes per fragment (a pool's buffer size), every datagram's last fragment
// half full on average.  512-byte buffers: MTU datagrams (3 fragments) ~427 B, nontemporal loads;
// IMIX (1.5 fragments) ~341 B, the temporal form with the tiny class — as the hint decides.
bool chain_nt_from_arena(uint64_t arena_bytes, uint32_t n_frags, double mean)
{
    const double frag_est = mean > 0.5 ? static_cast<double>(arena_bytes) / n_frags * (mean - 0.5) / mean : 0.0;
    return n_frags == 0 || frag_est >= RNS_CHAIN_NT_FROM;
}

// The temporal plain checksum (IMIX-like fragments) at 4 waves/SIMD for chains of 3+ packets
// per lane or 2+ fragments per packet (IMIX [492, 512, rest] chains 640 -> 598 us, IMIX
// transmit chains in 512-byte fragments 900 -> 790), else at 3 (IMIX in 512-byte NetBuffers
// 811 -> 754, [head, payload] chains 658 -> 620; session r05f, both forms free of scratch).
bool chain_deep(uint32_t K, double mean) { return K >= 3 || (K == 2 && mean >= 2.0); }

// Fragment chains: the chain kernel's launch (checksum or head-fragment fill) for set_chain's arguments.
template <bool FILL>
int chain_launch(CsumArgs &a, uint32_t frag_len_hint, hipStream_t stream)
{
    const double mean = chain_mean(a);
    a.chain_k = chain_pick_k(mean);
    // transmit-shaped chains: heads + a packed payload region.  A batch whose mean fragment
    // count already exceeds the shape (a head + kRunFrags payload fragments) has most of its
    // waves in the transmit-rows kernel's exact per-packet loop — far slower than the chain
    // kernel on the same chains — so the hint is ignored there (same results either way).
    if ((a.flags & RNS_FLAG_CHAIN_TX_PACKED) && mean <= 1.0 + kRunFrags)
        return launch_txrows<FILL>(a, stream);
    // RNS_FLAG_CHAIN_RUNS: the run-checking kernel (buffer path; a hint, ignored otherwise)
    const bool runs = kChainRuns && (a.flags & RNS_FLAG_CHAIN_RUNS) && buf_ok(a);
    return launch_chain<FILL>(a, a.chain_k, chain_nt_from_hint(frag_len_hint), runs, chain_deep(a.chain_k, mean), stream);
}

// Grid of the stash-mode kernels (one 64-datagram batch per one-wave workgroup).  Batches
// of tiny datagrams (arena bytes per datagram <= 128: ACK-sized) run on a capped grid, each
// wave looping over several batches: one-batch waves are mostly launch ramp there (64 B
// verify 18.9 -> 17.2-17.8 us per step); larger datagrams keep one wave per batch (a cap
// measured 3-6 % slower on IMIX; profiles/r02_rx_cap_ab.json).
constexpr uint64_t kRxGridCap = 4096;  // the cap for tiny datagrams
// Receive verify and transmit finalize take the cap (64 B finalize 35.2-36.3 -> 33.3 us);
// the single-field fill does not (64 B fill 28.9-29.2 us without, 29.8-30.0 with it:
// profiles/r02_tx_cap_ab.json).
dim3 stash_grid(uint64_t n, uint64_t arena_bytes, bool tiny_cap)
{
    constexpr int BLK = kMixedBlock<true>;
    uint64_t blocks = (waves64(n) + BLK / 64 - 1) / (BLK / 64);
    const bool cap = tiny_cap && arena_bytes / n <= 128;
    if (cap && blocks > kRxGridCap)
        blocks = kRxGridCap;
    return dim3(static_cast<uint32_t>(blocks));
}

bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// The pool receive form's arguments, as the verify and its consumers take them (buffers of 2^min_log2 bytes or more).
bool pool_rx_valid(const uint8_t *d_pool, uint32_t buf_log2, uint32_t min_log2, const uint32_t *d_buf_idx, uint32_t n_frags,
                   const uint32_t *d_blk_first, const uint16_t *d_len16, uint32_t n_pkts, const uint8_t *local_ipv4,
                   const uint8_t *local_ipv6, const uint8_t *d_status)
{
    return d_pool && buf_log2 >= min_log2 && buf_log2 <= kPoolMaxLog2 && d_blk_first && d_len16 && (!n_frags || d_buf_idx) &&
           n_pkts <= RNS_CHAIN_MAX_PACKETS && !misaligned(d_pool, 15) && rx_valid(d_status, local_ipv4, local_ipv6);
}

// A consumer's first step: the verify as it is (its kernel, its status and L4 sum), then the view of the
// verified batch and the load form for the consumer's kernels, picked as the verify picks its own.
int pool_rx_verify(PoolRx &rx, bool &nt, const uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2,
                   const uint32_t *d_buf_idx, uint32_t n_frags, const uint32_t *d_blk_first, const uint16_t *d_len16,
                   uint32_t n_pkts, const uint8_t *local_ipv4, const uint8_t *local_ipv6, uint8_t *d_status, uint16_t *d_l4_sum,
                   void *stream)
{
    RNS_TRY(rns_rx_verify_pool_dev(d_pool, pool_bytes, buf_log2, d_buf_idx, n_frags, d_blk_first, d_len16, n_pkts, local_ipv4,
                                   local_ipv6, d_status, d_l4_sum, stream));
    rx = PoolRx{d_pool, pool_bytes, d_buf_idx, d_blk_first, d_len16, d_status, n_pkts, n_frags, buf_log2};
    nt = chain_nt_from_arena(pool_bytes, n_frags, static_cast<double>(n_frags) / n_pkts);
    return RNS_OK;
}

// The pool transmit form's arguments, as its builders take them (cap: the datagrams the descriptors have room for).
bool pool_tx_valid(const uint8_t *d_tx_pool, const uint32_t *d_free, uint32_t n_free, uint32_t cap, const uint32_t *d_ip_id_add,
                   const uint32_t *d_tx_blk_first, const uint8_t *d_tx_head_len8, const uint16_t *d_tx_pay_len16,
                   const uint32_t *d_tx_src, const uint32_t *d_count)
{
    return d_tx_pool && d_count && (!n_free || d_free) && (!cap || (d_tx_blk_first && d_tx_head_len8 && d_tx_pay_len16)) &&
           !misaligned(d_tx_pool, 15) && !misaligned(d_free, 3) && !misaligned(d_ip_id_add, 3) &&
           !misaligned(d_tx_blk_first, 3) && !misaligned(d_tx_pay_len16, 1) && !misaligned(d_tx_src, 3) &&
           !misaligned(d_count, 3);
}

void set_pool_tx(PoolTx &tx, uint8_t *d_tx_pool, uint64_t tx_pool_bytes, uint32_t buf_log2, const uint32_t *d_free,
                 uint32_t n_free, uint32_t cap, uint16_t ip_id_base, const uint32_t *d_ip_id_add, uint32_t *d_tx_blk_first,
                 uint8_t *d_tx_head_len8, uint16_t *d_tx_pay_len16, uint32_t *d_tx_src, uint32_t *d_count)
{
    tx = PoolTx{d_tx_pool, tx_pool_bytes >> buf_log2, d_free, d_ip_id_add, d_tx_blk_first, d_tx_head_len8, d_tx_pay_len16,
                d_tx_src, d_count, n_free, cap, ip_id_base, buf_log2};
}

// An empty batch of an entry that leaves counts: the zeroed counts alone.
int count_only(uint32_t *d_count, size_t bytes, void *stream)
{
    if (!d_count || misaligned(d_count, 3))
        return RNS_E_INVALID;
    RNS_TRY(check_device());
    return launch_fill32(d_count, bytes / 4, 0u, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

int rns_csum_batch_dev_cfg(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_off,
                           const uint32_t *d_len, const uint16_t *d_seed, uint16_t *d_out, uint32_t n,
                           uint32_t flags, uint32_t variant, uint32_t lanes_per_packet, uint32_t unroll,
                           uint32_t max_blocks, uint32_t *d_bad, void *stream)
{
    return entry(n, d_off && d_len && d_out, d_arena, arena_bytes, flags, stream, [&](CsumArgs &a, hipStream_t st) {
        set_explicit(a, d_off, d_len);
        set_results(a, d_seed, d_out, d_bad);
        return dispatch<false>(a, variant, lanes_per_packet, unroll, max_blocks, st);
    });
}

int rns_csum_batch_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_off,
                       const uint32_t *d_len, const uint16_t *d_seed, uint16_t *d_out, uint32_t n,
                       uint32_t flags, uint32_t len_hint, uint32_t *d_bad, void *stream)
{
    const Shape sh = pick_shape(len_hint);
    return rns_csum_batch_dev_cfg(d_arena, arena_bytes, d_off, d_len, d_seed, d_out, n, flags, sh.variant, sh.G,
                                  sh.U, sh.max_blocks, d_bad, stream);
}

int rns_csum_batch_dev_off32(const uint8_t *d_arena, uint64_t arena_bytes, const uint32_t *d_off32,
                             const uint32_t *d_len, const uint16_t *d_seed, uint16_t *d_out, uint32_t n,
                             uint32_t flags, uint32_t len_hint, uint32_t *d_bad, void *stream)
{
    return entry(n, d_off32 && d_len && d_out, d_arena, arena_bytes, flags, stream, [&](CsumArgs &a, hipStream_t st) {
        a.off32 = d_off32;
        a.len = d_len;
        set_results(a, d_seed, d_out, d_bad);
        const Shape sh = pick_shape(len_hint);
        return dispatch<false>(a, sh.variant, sh.G, sh.U, sh.max_blocks, st);
    });
}

int rns_csum_batch_packed_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_blk_off,
                              const uint16_t *d_len16, uint32_t align_log2, const uint16_t *d_seed, uint16_t *d_out,
                              uint32_t n, uint32_t flags, uint32_t len_hint, uint32_t *d_bad, void *stream)
{
    return entry(n, d_blk_off && d_len16 && d_out && packed_align(align_log2, 0), d_arena, arena_bytes, flags, stream,
                 [&](CsumArgs &a, hipStream_t st) {
                     set_packed(a, d_blk_off, d_len16, align_log2);
                     set_results(a, d_seed, d_out, d_bad);
                     a.len_hint = len_hint;
                     Shape sh = pick_shape(len_hint);
                     if ((sh.variant & 5u) == 0)  // the group kernel has no 64-packet wave batches: mixed kernel, nontemporal
                         sh = Shape{6u, 0u, 0u, 0u};
                     return dispatch_packed(a, sh, st);
                 });
}

int rns_csum_batch_strided_dev(const uint8_t *d_arena, uint64_t arena_bytes, uint64_t first_off,
                               uint64_t stride, uint32_t len, const uint16_t *d_seed, uint16_t *d_out,
                               uint32_t n, uint32_t flags, uint32_t *d_bad, void *stream)
{
    return entry(n, d_out && strided_fits(first_off, stride, n), d_arena, arena_bytes, flags, stream,
                 [&](CsumArgs &a, hipStream_t st) {
                     set_strided(a, first_off, stride);
                     set_results(a, d_seed, d_out, d_bad);
                     a.fixed_len = len;
                     // packets of at most 64 bytes at 16-byte-aligned starts: the strided tiny kernel (c2 isolated
                     // 12.83-12.94 -> 12.24-12.29 us against the rounds kernel: sessions r05g, r05h)
                     if (len != 0 && len <= 64 && ((first_off + a.base_adjust) & 15) == 0 && (stride & 15) == 0)
                         return launch_strided_tiny(a, st);
                     const Shape sh = pick_shape(len);
                     return dispatch<true>(a, sh.variant, sh.G, sh.U, sh.max_blocks, st);
                 });
}

int rns_csum_chain_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_frag_off,
                       const uint32_t *d_frag_len, uint32_t n_frags, const uint32_t *d_first,
                       const uint16_t *d_seed, uint16_t *d_out, uint32_t n_pkts, uint32_t flags,
                       uint32_t frag_len_hint, uint16_t *d_frag_sums, uint32_t *d_bad, void *stream)
{
    (void)d_frag_sums;  // scratch of the two-pass form (round 1); the one-pass kernel needs none
    return entry(n_pkts, d_out && chain_valid(d_frag_off, d_frag_len, d_first, n_frags, n_pkts), d_arena, arena_bytes,
                 flags, stream, [&](CsumArgs &a, hipStream_t st) {
                     set_chain(a, d_frag_off, d_frag_len, d_first, n_frags);
                     set_results(a, d_seed, d_out, d_bad);
                     return chain_launch<false>(a, frag_len_hint, st);
                 });
}

int rns_csum_chain_fill_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_frag_off,
                            const uint32_t *d_frag_len, uint32_t n_frags, const uint32_t *d_first,
                            const uint16_t *d_seed, const uint16_t *d_field, uint32_t field_off, uint16_t *d_out,
                            uint32_t n_pkts, uint32_t flags, uint32_t frag_len_hint, uint32_t *d_bad, void *stream)
{
    return entry(n_pkts, chain_valid(d_frag_off, d_frag_len, d_first, n_frags, n_pkts), d_arena, arena_bytes, flags,
                 stream, [&](CsumArgs &a, hipStream_t st) {
                     set_chain(a, d_frag_off, d_frag_len, d_first, n_frags);
                     set_results(a, d_seed, d_out, d_bad);
                     set_field(a, d_field, field_off);
                     return chain_launch<true>(a, frag_len_hint, st);
                 });
}

int rns_csum_fill_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_off, const uint32_t *d_len,
                      const uint16_t *d_seed, const uint16_t *d_field, uint32_t field_off, uint16_t *d_out,
                      uint32_t n, uint32_t flags, uint32_t *d_bad, void *stream)
{
    return entry(n, d_off && d_len, d_arena, arena_bytes, flags, stream, [&](CsumArgs &a, hipStream_t st) {
        set_explicit(a, d_off, d_len);
        set_results(a, d_seed, d_out, d_bad);
        set_field(a, d_field, field_off);
        return launch_fill(a, stash_grid(n, arena_bytes, false), st);
    });
}

int rns_csum_fill_packed_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_blk_off, const uint16_t *d_len16,
                             uint32_t align_log2, const uint16_t *d_seed, const uint16_t *d_field, uint32_t field_off,
                             uint16_t *d_out, uint32_t n, uint32_t flags, uint32_t len_hint, uint32_t *d_bad,
                             void *stream)
{
    return entry(n, d_blk_off && d_len16 && packed_align(align_log2, 4), d_arena, arena_bytes, flags, stream,
                 [&](CsumArgs &a, hipStream_t st) {
                     set_packed(a, d_blk_off, d_len16, align_log2);
                     set_results(a, d_seed, d_out, d_bad);
                     set_field(a, d_field, field_off);
                     a.len_hint = len_hint;
                     return launch_fill_packed(a, st);
                 });
}

int rns_rx_verify_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_off, const uint32_t *d_len,
                      uint32_t n, const uint8_t *local_ipv4, const uint8_t *local_ipv6, uint8_t *d_status,
                      uint16_t *d_l4_sum, void *stream)
{
    return entry(n, d_off && d_len && rx_valid(d_status, local_ipv4, local_ipv6), d_arena, arena_bytes,
                 RNS_FLAG_COMPLEMENT, stream, [&](CsumArgs &a, hipStream_t st) {
                     set_explicit(a, d_off, d_len);
                     set_rx(a, d_status, d_l4_sum, local_ipv4, local_ipv6);
                     return launch_rx(a, stash_grid(n, arena_bytes, true), st);
                 });
}

int rns_rx_verify_packed_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_blk_off,
                             const uint16_t *d_len16, uint32_t align_log2, uint32_t n, const uint8_t *local_ipv4,
                             const uint8_t *local_ipv6, uint8_t *d_status, uint16_t *d_l4_sum, void *stream)
{
    return entry(n, d_blk_off && d_len16 && rx_valid(d_status, local_ipv4, local_ipv6) && packed_align(align_log2, 4),
                 d_arena, arena_bytes, RNS_FLAG_COMPLEMENT, stream, [&](CsumArgs &a, hipStream_t st) {
                     set_packed(a, d_blk_off, d_len16, align_log2);
                     set_rx(a, d_status, d_l4_sum, local_ipv4, local_ipv6);
                     return launch_stream_rx(a, st);
                 });
}

int rns_rx_verify_strided_dev(const uint8_t *d_arena, uint64_t arena_bytes, uint64_t first_off, uint64_t stride,
                              const uint16_t *d_len16, uint32_t n, const uint8_t *local_ipv4, const uint8_t *local_ipv6,
                              uint8_t *d_status, uint16_t *d_l4_sum, void *stream)
{
    return entry(n, d_len16 && rx_valid(d_status, local_ipv4, local_ipv6) && strided_fits(first_off, stride, n), d_arena,
                 arena_bytes, RNS_FLAG_COMPLEMENT, stream, [&](CsumArgs &a, hipStream_t st) {
                     a.len16 = d_len16;
                     set_strided(a, first_off, stride);
                     set_rx(a, d_status, d_l4_sum, local_ipv4, local_ipv6);
                     return launch_strided_rx(a, st);
                 });
}

int rns_rx_verify_chain_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_frag_off,
                            const uint32_t *d_frag_len, uint32_t n_frags, const uint32_t *d_first, uint32_t n_pkts,
                            const uint8_t *local_ipv4, const uint8_t *local_ipv6, uint8_t *d_status, uint16_t *d_l4_sum,
                            void *stream)
{
    return entry(n_pkts,
                 chain_valid(d_frag_off, d_frag_len, d_first, n_frags, n_pkts) &&
                     rx_valid(d_status, local_ipv4, local_ipv6),
                 d_arena, arena_bytes, RNS_FLAG_COMPLEMENT, stream, [&](CsumArgs &a, hipStream_t st) {
                     set_chain(a, d_frag_off, d_frag_len, d_first, n_frags);
                     set_rx(a, d_status, d_l4_sum, local_ipv4, local_ipv6);
                     const double mean = chain_mean(a);
                     a.chain_k = chain_pick_k(mean);
                     return launch_rx_chain(a, a.chain_k, chain_nt_from_arena(arena_bytes, n_frags, mean), st);
                 });
}

int rns_rx_verify_pool_dev(const uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2, const uint32_t *d_buf_idx,
                           uint32_t n_frags, const uint32_t *d_blk_first, const uint16_t *d_len16, uint32_t n_pkts,
                           const uint8_t *local_ipv4, const uint8_t *local_ipv6, uint8_t *d_status, uint16_t *d_l4_sum,
                           void *stream)
{
    return entry(n_pkts,
                 pool_rx_valid(d_pool, buf_log2, kPoolMinLog2, d_buf_idx, n_frags, d_blk_first, d_len16, n_pkts, local_ipv4,
                               local_ipv6, d_status),
                 d_pool, pool_bytes, RNS_FLAG_COMPLEMENT, stream, [&](CsumArgs &a, hipStream_t st) {
                     // the compact descriptors in CsumArgs: off32 = buffer indices, first = d_blk_first,
                     // len16 = datagram lengths, align_mask = buffer bytes - 1 (rns_k_pool_rx.hpp)
                     a.off32 = d_buf_idx;
                     a.n_frags = n_frags;
                     a.first = d_blk_first;
                     a.len16 = d_len16;
                     a.align_mask = (1u << buf_log2) - 1u;
                     set_rx(a, d_status, d_l4_sum, local_ipv4, local_ipv6);
                     const double mean = chain_mean(a);
                     a.chain_k = chain_pick_k(mean);
                     return launch_rx_pool(a, a.chain_k, chain_nt_from_arena(pool_bytes, n_frags, mean), st);
                 });
}

int rns_rx_tcp_place_pool_dev(const uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2, const uint32_t *d_buf_idx,
                              uint32_t n_frags, const uint32_t *d_blk_first, const uint16_t *d_len16, uint32_t n_pkts,
                              const uint8_t *local_ipv4, const uint8_t *local_ipv6, const uint8_t *d_tbl,
                              uint64_t tbl_bytes, const uint32_t *d_next_seq, const uint64_t *d_win_off,
                              const uint32_t *d_win_len, uint32_t n_flows, uint8_t *d_stream, uint64_t stream_bytes,
                              uint8_t *d_status, uint16_t *d_l4_sum, rns_rx_tcp_meta *d_meta, void *stream)
{
    static_assert(sizeof(rns_rx_tcp_meta) == 24 && sizeof(rns_rx_flow_key) == kFlowSlotBytes - 8, "rns_k_pool_place.hpp");
    if (n_pkts == 0)
        return RNS_OK;
    const uint64_t slots = flow_slots(n_flows);
    // every rejection of the verify's and this entry's own, before the device is touched
    if (!pool_rx_valid(d_pool, buf_log2, kPlaceMinLog2, d_buf_idx, n_frags, d_blk_first, d_len16, n_pkts, local_ipv4,
                       local_ipv6, d_status) ||
        !d_meta || misaligned(d_meta, 3) || !d_next_seq || !d_win_off || !d_win_len || !d_stream ||
        (n_flows && (!d_tbl || misaligned(d_tbl, 3) || tbl_bytes < slots * kFlowSlotBytes)))
        return RNS_E_INVALID;
    PoolRx rx;
    bool nt;
    RNS_TRY(pool_rx_verify(rx, nt, d_pool, pool_bytes, buf_log2, d_buf_idx, n_frags, d_blk_first, d_len16, n_pkts,
                           local_ipv4, local_ipv6, d_status, d_l4_sum, stream));
    const PlaceArgs p{rx.pool, rx.pool_bytes, rx.buf_idx, rx.blk_first, rx.len16, rx.status,  // the view, flat
                      reinterpret_cast<const uint32_t *>(d_tbl), d_next_seq, d_win_off, d_win_len, d_stream, stream_bytes,
                      reinterpret_cast<uint32_t *>(d_meta), rx.n, rx.n_frags, n_flows, static_cast<uint32_t>(slots), rx.blog};
    return launch_rx_place(p, nt, static_cast<hipStream_t>(stream));
}

int rns_rx_tcp_listen_pool_dev(const uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2, const uint32_t *d_buf_idx,
                               uint32_t n_frags, const uint32_t *d_blk_first, const uint16_t *d_len16, uint32_t n_pkts,
                               const uint8_t *local_ipv4, const uint8_t *local_ipv6, const rns_rx_tcp_meta *d_meta,
                               const uint16_t *d_listen, uint32_t n_listen, const uint32_t *d_iss, uint16_t ip_id_base,
                               const uint32_t *d_ip_id_add, uint8_t *d_out, uint32_t reply_cap, uint32_t *d_rep_src,
                               uint8_t *d_rep_len8, rns_tcp_accept *d_accept, uint32_t *d_count, uint8_t *d_conn, void *d_work,
                               uint64_t work_bytes, void *stream)
{
    static_assert(sizeof(rns_tcp_accept) == 72 && sizeof(rns_rx_flow_key) == 24 && sizeof(rns_tcp_flow) == 40,
                  "rns_k_listen.hpp: an accept record is 18 dwords");
    if (n_listen > RNS_UDP_MAX_SOCKS || !d_count || misaligned(d_count, 3))
        return RNS_E_INVALID;
    if (n_pkts == 0)  // no datagram: the counts alone
        return count_only(d_count, 12, stream);
    // every rejection, before the device is touched
    if (!d_pool || buf_log2 < kPlaceMinLog2 || buf_log2 > kPoolMaxLog2 || !d_blk_first || !d_len16 || (n_frags && !d_buf_idx) ||
        n_pkts > RNS_CHAIN_MAX_PACKETS || misaligned(d_pool, 15) || !local_ipv4 || !local_ipv6 || !d_meta || !d_conn ||
        !d_work || (n_listen && !d_listen) || (reply_cap && (!d_out || !d_rep_src || !d_rep_len8 || !d_accept || !d_iss)) ||
        misaligned(d_meta, 3) || misaligned(d_listen, 1) || misaligned(d_iss, 3) || misaligned(d_ip_id_add, 3) ||
        misaligned(d_out, 3) || misaligned(d_rep_src, 3) || misaligned(d_accept, 3) || misaligned(d_work, 7) ||
        work_bytes < listen_work_bytes(n_pkts))
        return RNS_E_INVALID;
    RNS_TRY(check_device());
    ListenArgs a{};
    a.rx = PoolRx{d_pool, pool_bytes, d_buf_idx, d_blk_first, d_len16, nullptr, n_pkts, n_frags, buf_log2};
    a.meta = reinterpret_cast<const uint32_t *>(d_meta);
    a.listen = d_listen;
    a.iss = d_iss;
    a.ip_id_add = d_ip_id_add;
    a.out = d_out;
    a.rep_src = d_rep_src;
    a.rep_len8 = d_rep_len8;
    a.accept = reinterpret_cast<uint32_t *>(d_accept);
    a.count = d_count;
    a.conn = d_conn;
    a.slots = flow_slots(n_pkts);
    a.tbl = static_cast<unsigned long long *>(d_work);
    a.first = reinterpret_cast<uint32_t *>(a.tbl + a.slots);
    a.w = carve_build_work(a.first + a.slots, n_pkts);  // (12 * slots bytes on: 8-byte aligned)
    set_local(a.local, local_ipv4, local_ipv6);
    a.n_listen = n_listen;
    a.reply_cap = reply_cap;
    a.ip_id_base = ip_id_base;
    return launch_rx_listen(a, static_cast<hipStream_t>(stream));
}

int rns_rx_icmp_echo_pool_dev(const uint8_t *d_rx_pool, uint64_t rx_pool_bytes, uint32_t buf_log2,
                              const uint32_t *d_buf_idx, uint32_t n_frags, const uint32_t *d_blk_first,
                              const uint16_t *d_len16, uint32_t n_pkts, const uint8_t *local_ipv4,
                              const uint8_t *local_ipv6, uint8_t *d_tx_pool, uint64_t tx_pool_bytes, const uint32_t *d_free,
                              uint32_t n_free, uint32_t reply_cap, uint16_t ip_id_base, const uint32_t *d_ip_id_add,
                              uint32_t *d_tx_blk_first, uint8_t *d_tx_head_len8, uint16_t *d_tx_pay_len16,
                              uint32_t *d_tx_src, uint32_t *d_count, uint8_t *d_status, uint16_t *d_l4_sum, uint8_t *d_echo,
                              void *d_work, uint64_t work_bytes, void *stream)
{
    if (n_pkts == 0)  // no datagram: the counts alone
        return count_only(d_count, 12, stream);
    // every rejection of the verify's and this entry's own, before the device is touched
    if (!pool_rx_valid(d_rx_pool, buf_log2, kEchoMinLog2, d_buf_idx, n_frags, d_blk_first, d_len16, n_pkts, local_ipv4,
                       local_ipv6, d_status) ||
        !pool_tx_valid(d_tx_pool, d_free, n_free, reply_cap, d_ip_id_add, d_tx_blk_first, d_tx_head_len8, d_tx_pay_len16,
                       d_tx_src, d_count) ||
        !d_echo || !d_work || misaligned(d_work, 7) || work_bytes < echo_work_bytes(n_pkts))
        return RNS_E_INVALID;
    EchoArgs a{};
    bool nt;
    RNS_TRY(pool_rx_verify(a.rx, nt, d_rx_pool, rx_pool_bytes, buf_log2, d_buf_idx, n_frags, d_blk_first, d_len16, n_pkts,
                           local_ipv4, local_ipv6, d_status, d_l4_sum, stream));
    set_pool_tx(a.tx, d_tx_pool, tx_pool_bytes, buf_log2, d_free, n_free, reply_cap, ip_id_base, d_ip_id_add, d_tx_blk_first,
                d_tx_head_len8, d_tx_pay_len16, d_tx_src, d_count);
    a.w = carve_build_work(d_work, n_pkts);
    set_local(a.local, local_ipv4, local_ipv6);
    a.echo = d_echo;
    return launch_rx_echo(a, nt, static_cast<hipStream_t>(stream));
}

int rns_rx_udp_demux_pool_dev(const uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2, const uint32_t *d_buf_idx,
                              uint32_t n_frags, const uint32_t *d_blk_first, const uint16_t *d_len16, uint32_t n_pkts,
                              const uint8_t *local_ipv4, const uint8_t *local_ipv6, const uint16_t *d_port_tbl,
                              uint32_t n_socks, uint8_t *d_data, uint64_t data_bytes, rns_udp_rec *d_rec, uint32_t rec_cap,
                              uint32_t *d_q_first, uint32_t *d_count, uint8_t *d_status, uint16_t *d_l4_sum, uint8_t *d_udp,
                              uint32_t *d_pos, void *d_work, uint64_t work_bytes, void *stream)
{
    static_assert(sizeof(rns_udp_rec) == 32, "rns_k_udp.hpp: a record is two 16-byte stores");
    if (n_socks > RNS_UDP_MAX_SOCKS || !d_q_first || !d_count || misaligned(d_q_first, 3) || misaligned(d_count, 3))
        return RNS_E_INVALID;
    if (n_pkts == 0) {  // no datagram: the counts and the empty queues alone
        RNS_TRY(check_device());
        RNS_TRY(launch_fill32(d_count, 2, 0u, static_cast<hipStream_t>(stream)));
        return launch_fill32(d_q_first, n_socks + 1ull, 0u, static_cast<hipStream_t>(stream));
    }
    // every rejection of the verify's and this entry's own, before the device is touched
    if (!pool_rx_valid(d_pool, buf_log2, kUdpMinLog2, d_buf_idx, n_frags, d_blk_first, d_len16, n_pkts, local_ipv4, local_ipv6,
                       d_status) ||
        !d_udp || !d_work || (n_socks && !d_port_tbl) || (data_bytes && !d_data) || (rec_cap && !d_rec) ||
        misaligned(d_data, 15) || misaligned(d_rec, 15) || misaligned(d_work, 15) || misaligned(d_port_tbl, 1) ||
        misaligned(d_pos, 3) || work_bytes < udp_work_bytes(n_pkts, n_socks) ||
        (static_cast<uint64_t>(n_frags) << buf_log2) >= (1ull << 36))
        return RNS_E_INVALID;
    UdpArgs a{};
    bool nt;
    RNS_TRY(pool_rx_verify(a.rx, nt, d_pool, pool_bytes, buf_log2, d_buf_idx, n_frags, d_blk_first, d_len16, n_pkts, local_ipv4,
                           local_ipv6, d_status, d_l4_sum, stream));
    a.port_tbl = d_port_tbl;
    a.data = d_data;
    a.data_bytes = data_bytes;
    a.rec_out = reinterpret_cast<uint4 *>(d_rec);
    a.q_first = d_q_first;
    a.count = d_count;
    a.udp = d_udp;
    a.pos = d_pos;
    a.n_socks = n_socks;
    a.n_tiles = static_cast<uint32_t>(udp_tiles(n_pkts));
    a.rec_cap = rec_cap;
    const uint64_t m = static_cast<uint64_t>(n_socks) * a.n_tiles;
    a.part = static_cast<uint2 *>(d_work);
    a.mat = a.part + scan_blocks(m) + 1;
    a.rec = reinterpret_cast<uint32_t *>(a.mat + m);
    return launch_rx_udp(a, nt, static_cast<hipStream_t>(stream));
}

int rns_tx_udp_send_pool_dev(const uint8_t *d_data, uint64_t data_bytes, const rns_udp_rec *d_rec, uint32_t n_recs,
                             const uint32_t *d_q_first, const uint16_t *d_sock_port, uint32_t n_socks,
                             const uint8_t *local_ipv4, const uint8_t *local_ipv6, uint8_t *d_tx_pool,
                             uint64_t tx_pool_bytes, uint32_t buf_log2, const uint32_t *d_free, uint32_t n_free,
                             uint32_t send_cap, uint16_t ip_id_base, const uint32_t *d_ip_id_add, uint32_t *d_tx_blk_first,
                             uint8_t *d_tx_head_len8, uint16_t *d_tx_pay_len16, uint32_t *d_tx_src, uint32_t *d_count,
                             uint8_t *d_send, void *d_work, uint64_t work_bytes, void *stream)
{
    static_assert(sizeof(rns_udp_rec) == 32, "rns_k_udp_tx.hpp: a record is two 16-byte loads");
    if (n_recs == 0)  // no record: the counts alone
        return count_only(d_count, 12, stream);
    // every rejection, before the device is touched
    if (buf_log2 < kUdpTxMinLog2 || buf_log2 > kPoolMaxLog2 || n_recs > RNS_CHAIN_MAX_PACKETS || n_socks == 0 ||
        n_socks > RNS_UDP_MAX_SOCKS || !d_data || !d_rec || !d_q_first || !d_sock_port || !local_ipv4 || !local_ipv6 ||
        !pool_tx_valid(d_tx_pool, d_free, n_free, send_cap, d_ip_id_add, d_tx_blk_first, d_tx_head_len8, d_tx_pay_len16,
                       d_tx_src, d_count) ||
        !d_send || !d_work || misaligned(d_data, 15) || misaligned(d_rec, 15) || misaligned(d_q_first, 3) ||
        misaligned(d_sock_port, 1) || misaligned(d_work, 7) || work_bytes < udp_tx_work_bytes(n_recs))
        return RNS_E_INVALID;
    RNS_TRY(check_device());
    UdpTxArgs a{};
    a.data = d_data;
    a.data_bytes = data_bytes;
    a.rec_in = reinterpret_cast<const uint4 *>(d_rec);
    a.q_first = d_q_first;
    a.sock_port = d_sock_port;
    set_pool_tx(a.tx, d_tx_pool, tx_pool_bytes, buf_log2, d_free, n_free, send_cap, ip_id_base, d_ip_id_add, d_tx_blk_first,
                d_tx_head_len8, d_tx_pay_len16, d_tx_src, d_count);
    a.w = carve_build_work(d_work, n_recs);
    set_local(a.local, local_ipv4, local_ipv6);
    a.send = d_send;
    a.n_recs = n_recs;
    a.n_socks = n_socks;
    return launch_tx_udp(a, static_cast<hipStream_t>(stream));
}

// The flow update's and the connection update's one validation and marshalling: d_rec = d_seg or d_ctl.
static int flow_walk_args(FlowArgs &a, const rns_rx_tcp_meta *d_meta, uint32_t n_pkts, uint32_t n_flows,
                          const rns_tcp_flow *d_flow_in, const uint32_t *d_pend_in, uint32_t pend_cap, rns_tcp_flow *d_flow_out,
                          uint32_t *d_pend_out, void *d_rec, rns_tcp_flow_res *d_res, void *d_work, uint64_t work_bytes)
{
    static_assert(sizeof(rns_tcp_flow) == 4 * kFlowDw && sizeof(rns_rx_tcp_seg) == 8 && sizeof(rns_tcp_ctl) == 4 * kCtlDw &&
                      sizeof(rns_tcp_flow_res) == 4 * kFlowResDw,
                  "rns_k_args.hpp");
    const bool pend = n_flows && pend_cap;
    if (n_pkts > RNS_CHAIN_MAX_PACKETS || n_flows > kFlowMaxFlows || (n_pkts && (!d_meta || !d_rec)) ||
        (n_flows && (!d_flow_in || !d_flow_out || !d_res)) || (pend && (!d_pend_in || !d_pend_out)) || !d_work ||
        misaligned(d_meta, 3) || misaligned(d_rec, 3) || misaligned(d_flow_in, 3) || misaligned(d_flow_out, 3) ||
        misaligned(d_res, 3) || (pend && (misaligned(d_pend_in, 3) || misaligned(d_pend_out, 3))) || misaligned(d_work, 7) ||
        work_bytes < flow_work_bytes(n_pkts, n_flows))
        return RNS_E_INVALID;
    RNS_TRY(check_device());
    a.meta = reinterpret_cast<const uint32_t *>(d_meta);
    a.flow_in = reinterpret_cast<const uint32_t *>(d_flow_in);
    a.pend_in = d_pend_in;
    a.flow_out = reinterpret_cast<uint32_t *>(d_flow_out);
    a.pend_out = d_pend_out;
    a.rec = static_cast<uint32_t *>(d_rec);
    a.res = reinterpret_cast<uint32_t *>(d_res);
    a.part = static_cast<uint2 *>(d_work);
    a.cnt = static_cast<uint32_t *>(d_work) + 2 * (scan_blocks(n_flows) + 1);
    a.cursor = a.cnt + n_flows;
    a.longs = a.cursor + n_flows;
    a.list = a.longs + n_flows;
    a.n_pkts = n_pkts;
    a.n_flows = n_flows;
    a.pend_cap = pend_cap;
    return RNS_OK;
}

int rns_rx_tcp_flow_update_dev(const rns_rx_tcp_meta *d_meta, uint32_t n_pkts, uint32_t n_flows,
                               const rns_tcp_flow *d_flow_in, const uint32_t *d_pend_in, uint32_t pend_cap,
                               rns_tcp_flow *d_flow_out, uint32_t *d_pend_out, rns_rx_tcp_seg *d_seg,
                               rns_tcp_flow_res *d_res, void *d_work, uint64_t work_bytes, void *stream)
{
    if (n_pkts == 0 && n_flows == 0)
        return RNS_OK;
    FlowArgs a{};
    RNS_TRY(flow_walk_args(a, d_meta, n_pkts, n_flows, d_flow_in, d_pend_in, pend_cap, d_flow_out, d_pend_out, d_seg, d_res, d_work,
                           work_bytes));
    return launch_flow_update(a, static_cast<hipStream_t>(stream));
}

int rns_rx_tcp_conn_update_dev(const rns_rx_tcp_meta *d_meta, uint32_t n_pkts, uint32_t n_flows,
                               const rns_tcp_flow *d_flow_in, const uint32_t *d_pend_in, uint32_t pend_cap,
                               rns_tcp_flow *d_flow_out, uint32_t *d_pend_out, rns_tcp_ctl *d_ctl, rns_tcp_flow_res *d_res,
                               void *d_work, uint64_t work_bytes, void *stream)
{
    if (n_pkts == 0 && n_flows == 0)
        return RNS_OK;
    FlowArgs a{};
    RNS_TRY(flow_walk_args(a, d_meta, n_pkts, n_flows, d_flow_in, d_pend_in, pend_cap, d_flow_out, d_pend_out, d_ctl, d_res, d_work,
                           work_bytes));
    return launch_conn_update(a, static_cast<hipStream_t>(stream));
}

int rns_tx_tcp_ctl_build_dev(const rns_tcp_ctl *d_ctl, uint32_t n_ctl, uint32_t n_flows, const uint8_t *d_tmpl,
                             uint32_t tmpl_stride, const uint8_t *d_head_len8, uint16_t ip_id_base, const uint32_t *d_ip_id_add,
                             void *d_work, uint64_t work_bytes, uint8_t *d_out, uint32_t out_cap, uint32_t *d_src,
                             uint8_t *d_len8, uint32_t *d_count, void *stream)
{
    if (!d_count || n_ctl > RNS_CHAIN_MAX_PACKETS || (n_ctl && (!d_ctl || !d_work || work_bytes < ctl_work_bytes(n_ctl))) ||
        (n_ctl && n_flows && (!d_tmpl || !d_head_len8 || !tmpl_stride)) || (out_cap && (!d_out || !d_src || !d_len8)) ||
        misaligned(d_ctl, 3) || misaligned(d_ip_id_add, 3) || misaligned(d_out, 3) || misaligned(d_src, 3) ||
        misaligned(d_count, 3) || misaligned(d_work, 7))
        return RNS_E_INVALID;
    RNS_TRY(check_device());
    CtlArgs a{};
    a.ctl = reinterpret_cast<const uint32_t *>(d_ctl);
    a.tmpl = d_tmpl;
    a.head_len8 = d_head_len8;
    a.ip_id_add = d_ip_id_add;
    a.out = d_out;
    a.src = d_src;
    a.len8 = d_len8;
    a.count = d_count;
    a.part = static_cast<uint2 *>(d_work);
    a.n_ctl = n_ctl;
    a.n_flows = n_flows;
    a.tmpl_stride = tmpl_stride;
    a.ip_id_base = ip_id_base;
    a.out_cap = out_cap;
    return launch_ctl_build(a, static_cast<hipStream_t>(stream));
}

int rns_tx_tcp_close_dev(const rns_tcp_flow *d_flow_in, rns_tcp_flow *d_flow_out, uint32_t n_flows, const uint8_t *d_op,
                         rns_tcp_ctl *d_ctl, void *stream)
{
    if (n_flows == 0)
        return RNS_OK;
    if (n_flows > kFlowMaxFlows || !d_flow_in || !d_flow_out || !d_op || !d_ctl || misaligned(d_flow_in, 3) ||
        misaligned(d_flow_out, 3) || misaligned(d_ctl, 3))
        return RNS_E_INVALID;
    RNS_TRY(check_device());
    const CloseArgs a{reinterpret_cast<const uint32_t *>(d_flow_in), reinterpret_cast<uint32_t *>(d_flow_out), d_op,
                      reinterpret_cast<uint32_t *>(d_ctl), n_flows};
    return launch_conn_close(a, static_cast<hipStream_t>(stream));
}

int rns_tx_ack_build_dev(const rns_rx_tcp_meta *d_meta, const rns_rx_tcp_seg *d_seg, uint32_t n_pkts,
                         const rns_tcp_flow *d_flow, uint32_t n_flows, const uint8_t *d_tmpl, uint32_t tmpl_stride,
                         const uint8_t *d_head_len8, uint16_t ip_id_base, void *d_work, uint64_t work_bytes,
                         uint8_t *d_out, uint32_t ack_cap, uint32_t *d_ack_src, uint8_t *d_ack_len8, uint32_t *d_n_acks,
                         void *stream)
{
    if (!d_n_acks || n_pkts > RNS_CHAIN_MAX_PACKETS ||
        (n_pkts && (!d_meta || !d_seg || !d_work || work_bytes < ack_work_bytes(n_pkts))) ||
        (n_pkts && n_flows && (!d_flow || !d_tmpl || !d_head_len8 || !tmpl_stride)) ||
        (ack_cap && (!d_out || !d_ack_src || !d_ack_len8)) || misaligned(d_meta, 3) || misaligned(d_seg, 3) ||
        misaligned(d_flow, 3) || misaligned(d_out, 3) || misaligned(d_ack_src, 3) || misaligned(d_n_acks, 3) ||
        misaligned(d_work, 7))
        return RNS_E_INVALID;
    RNS_TRY(check_device());
    AckArgs a{};
    a.meta = reinterpret_cast<const uint32_t *>(d_meta);
    a.seg = reinterpret_cast<const uint32_t *>(d_seg);
    a.flow = reinterpret_cast<const uint32_t *>(d_flow);
    a.tmpl = d_tmpl;
    a.head_len8 = d_head_len8;
    a.out = d_out;
    a.ack_src = d_ack_src;
    a.ack_len8 = d_ack_len8;
    a.n_acks = d_n_acks;
    a.part = static_cast<uint2 *>(d_work);
    a.n_pkts = n_pkts;
    a.n_flows = n_flows;
    a.tmpl_stride = tmpl_stride;
    a.ip_id_base = ip_id_base;
    a.ack_cap = ack_cap;
    return launch_ack_build(a, static_cast<hipStream_t>(stream));
}

int rns_tx_tcp_plan_dev(const rns_tcp_flow *d_flow_in, rns_tcp_flow *d_flow_out, uint32_t n_flows, const uint64_t *d_sq_off,
                        const uint32_t *d_sq_seq, const uint32_t *d_sq_len, const uint16_t *d_mss, const uint8_t *d_rexmit,
                        const uint8_t *d_tmpl, uint32_t tmpl_stride, const uint8_t *d_head_len8, uint16_t ip_id_base,
                        const uint32_t *d_ip_id_add, uint64_t head_first_off, uint32_t seg_cap, uint8_t *d_tmpl_out,
                        uint8_t *d_head_len8_out, uint64_t *d_pay_off, uint32_t *d_pay_len, uint16_t *d_mss_out,
                        uint64_t *d_head_off, uint32_t *d_seg_first, uint32_t *d_blk_flow, uint32_t *d_n,
                        rns_tx_plan_res *d_res, void *d_work, uint64_t work_bytes, void *stream)
{
    static_assert(sizeof(rns_tx_plan_res) == 4 * kPlanResDw, "rns_k_args.hpp");
    if (n_flows > kPlanMaxFlows || seg_cap > RNS_CHAIN_MAX_PACKETS || !tmpl_stride || !d_seg_first || !d_n ||
        (seg_cap && !d_blk_flow) ||
        (n_flows && (!d_flow_in || !d_flow_out || !d_sq_off || !d_sq_seq || !d_sq_len || !d_mss || !d_tmpl || !d_head_len8 ||
                     !d_tmpl_out || !d_head_len8_out || !d_pay_off || !d_pay_len || !d_mss_out || !d_head_off || !d_res ||
                     !d_work || work_bytes < plan_work_bytes(n_flows))) ||
        misaligned(d_flow_in, 3) || misaligned(d_flow_out, 3) || misaligned(d_sq_off, 7) || misaligned(d_sq_seq, 3) ||
        misaligned(d_sq_len, 3) || misaligned(d_mss, 1) || misaligned(d_ip_id_add, 3) || misaligned(d_pay_off, 7) ||
        misaligned(d_pay_len, 3) || misaligned(d_mss_out, 1) || misaligned(d_head_off, 7) || misaligned(d_seg_first, 3) ||
        misaligned(d_blk_flow, 3) || misaligned(d_n, 3) || misaligned(d_res, 3) || misaligned(d_work, 7))
        return RNS_E_INVALID;
    RNS_TRY(check_device());
    PlanArgs a{};
    a.flow_in = reinterpret_cast<const uint32_t *>(d_flow_in);
    a.flow_out = reinterpret_cast<uint32_t *>(d_flow_out);
    a.sq_off = d_sq_off;
    a.sq_seq = d_sq_seq;
    a.sq_len = d_sq_len;
    a.mss = d_mss;
    a.rexmit = d_rexmit;
    a.tmpl = d_tmpl;
    a.head_len8 = d_head_len8;
    a.ip_id_add = d_ip_id_add;
    a.tmpl_out = d_tmpl_out;
    a.head_len8_out = d_head_len8_out;
    a.pay_off = d_pay_off;
    a.pay_len = d_pay_len;
    a.mss_out = d_mss_out;
    a.head_off = d_head_off;
    a.seg_first = d_seg_first;
    a.blk_flow = d_blk_flow;
    a.n_out = d_n;
    a.res = reinterpret_cast<uint32_t *>(d_res);
    a.part = static_cast<uint2 *>(d_work);
    a.rec = a.part + scan_blocks(2ull * n_flows) + 2;
    a.head_first_off = head_first_off;
    a.n_flows = n_flows;
    a.tmpl_stride = tmpl_stride;
    a.ip_id_base = ip_id_base;
    a.seg_cap = seg_cap;
    return launch_tx_plan(a, static_cast<hipStream_t>(stream));
}

int rns_tx_fill_packed_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_blk_off, const uint16_t *d_len16,
                           uint32_t align_log2, uint32_t n, uint8_t *d_status, uint32_t len_hint, void *stream)
{
    return entry(n, d_blk_off && d_len16 && packed_align(align_log2, 4), d_arena, arena_bytes, RNS_FLAG_COMPLEMENT,
                 stream, [&](CsumArgs &a, hipStream_t st) {
                     set_packed(a, d_blk_off, d_len16, align_log2);
                     set_tx_status(a, d_status);
                     a.len_hint = len_hint;
                     return launch_tx_packed(a, st);
                 });
}

int rns_tx_fill_chain_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_frag_off, const uint32_t *d_frag_len,
                          uint32_t n_frags, const uint32_t *d_first, uint32_t n_pkts, uint8_t *d_status, void *stream)
{
    return entry(n_pkts, chain_valid(d_frag_off, d_frag_len, d_first, n_frags, n_pkts), d_arena, arena_bytes,
                 RNS_FLAG_COMPLEMENT, stream, [&](CsumArgs &a, hipStream_t st) {
                     set_chain(a, d_frag_off, d_frag_len, d_first, n_frags);
                     set_tx_status(a, d_status);
                     return launch_txrows<false, true>(a, st);
                 });
}

int rns_tx_fill_chain_packed_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_head_blk_off,
                                 const uint8_t *d_head_len8, const uint64_t *d_pay_blk_off, const uint16_t *d_pay_len16,
                                 uint32_t pay_align_log2, uint32_t n, uint8_t *d_status, void *stream)
{
    return entry(n,
                 d_head_blk_off && d_head_len8 && d_pay_blk_off && d_pay_len16 && packed_align(pay_align_log2, 4) &&
                     n <= RNS_CHAIN_MAX_PACKETS,
                 d_arena, arena_bytes, RNS_FLAG_COMPLEMENT, stream, [&](CsumArgs &a, hipStream_t st) {
                     a.head_blk_off = d_head_blk_off;
                     a.head_len8 = d_head_len8;
                     set_packed(a, d_pay_blk_off, d_pay_len16, pay_align_log2);
                     set_tx_status(a, d_status);
                     return launch_txrows<false, true, true>(a, st);
                 });
}

int rns_tx_fill_pool_dev(uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2, const uint32_t *d_buf_idx,
                         uint32_t n_frags, const uint32_t *d_blk_first, const uint8_t *d_head_len8,
                         const uint16_t *d_pay_len16, uint32_t n_pkts, uint8_t *d_status, void *stream)
{
    return entry(n_pkts,
                 buf_log2 >= kPoolTxMinLog2 && buf_log2 <= kPoolMaxLog2 && d_blk_first && d_head_len8 && d_pay_len16 &&
                     (!n_frags || d_buf_idx) && n_pkts <= RNS_CHAIN_MAX_PACKETS &&
                     (reinterpret_cast<uintptr_t>(d_pool) & 15) == 0,
                 d_pool, pool_bytes, RNS_FLAG_COMPLEMENT, stream, [&](CsumArgs &a, hipStream_t st) {
                     // the compact descriptors in CsumArgs: off32 = buffer indices, first = d_blk_first, head_len8,
                     // len16 = payload lengths, align_mask = buffer bytes - 1 (rns_k_pool_tx.hpp)
                     a.off32 = d_buf_idx;
                     a.n_frags = n_frags;
                     a.first = d_blk_first;
                     a.head_len8 = d_head_len8;
                     a.len16 = d_pay_len16;
                     a.align_mask = (1u << buf_log2) - 1u;
                     set_tx_status(a, d_status);
                     const double mean = chain_mean(a);
                     a.chain_k = chain_pick_k(mean);
                     return launch_tx_pool(a, a.chain_k, chain_nt_from_arena(pool_bytes, n_frags, mean), st);
                 });
}

int rns_tx_segment_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint8_t *d_tmpl, uint32_t tmpl_stride,
                       const uint8_t *d_head_len8, const uint64_t *d_pay_off, const uint32_t *d_pay_len,
                       const uint16_t *d_mss, const uint64_t *d_head_off, const uint32_t *d_seg_first,
                       const uint32_t *d_blk_flow, uint32_t n_flows, uint32_t n_seg, uint8_t *d_status, void *stream)
{
    return entry(n_flows ? n_seg : 0u,
                 d_tmpl && tmpl_stride && d_head_len8 && d_pay_off && d_pay_len && d_mss && d_head_off && d_seg_first &&
                     d_blk_flow && n_seg <= RNS_CHAIN_MAX_PACKETS,
                 d_arena, arena_bytes, RNS_FLAG_COMPLEMENT, stream, [&](CsumArgs &a, hipStream_t st) {
                     // the flows' descriptors in CsumArgs: first = d_seg_first, len = the data lengths, len16 = the
                     // mss, head_len8, and the fields of its own (rns_k_segment.hpp)
                     a.tmpl = d_tmpl;
                     a.tmpl_stride = tmpl_stride;
                     a.n_flows = n_flows;
                     a.head_len8 = d_head_len8;
                     a.seg_pay_off = d_pay_off;
                     a.len = d_pay_len;
                     a.len16 = d_mss;
                     a.seg_head_off = d_head_off;
                     a.first = d_seg_first;
                     a.blk_flow = d_blk_flow;
                     set_tx_status(a, d_status);
                     // nontemporal loads for MTU-sized segments, as the chain forms choose them
                     return launch_tx_segment(a, arena_bytes / n_seg >= RNS_CHAIN_NT_FROM, st);
                 });
}

int rns_tx_fill_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_off, const uint32_t *d_len,
                    uint32_t n, uint8_t *d_status, void *stream)
{
    return entry(n, d_off && d_len, d_arena, arena_bytes, RNS_FLAG_COMPLEMENT, stream, [&](CsumArgs &a, hipStream_t st) {
        set_explicit(a, d_off, d_len);
        set_tx_status(a, d_status);
        return launch_tx(a, stash_grid(n, arena_bytes, true), st);
    });
}

int rns_fill_splitmix64_dev(uint8_t *d_buf, uint64_t nbytes, uint64_t seed, void *stream)
{
    if (nbytes == 0)
        return RNS_OK;
    if (!d_buf || (reinterpret_cast<uintptr_t>(d_buf) & 7))
        return RNS_E_INVALID;
    RNS_TRY(check_device());
    const uint64_t words = (nbytes + 7) / 8;
    const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((words + kBlock - 1) / kBlock, 8192));
    hipLaunchKernelGGL(splitmix64_fill_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       d_buf, nbytes, seed);
    return hip_status(hipGetLastError());
}

const char *rns_csum_shape_name(uint32_t len_hint)
{
    static const char *const names[] = {"csum_batch_kernel",     "csum_rounds_kernel",     "csum_batch_kernel[nt]",
                                        "csum_rounds_kernel[nt]", "csum_mixed_kernel",      "csum_mixed_kernel",
                                        "csum_mixed_kernel[nt]",  "csum_mixed_kernel[nt]"};
    static thread_local char buf[96];
    const Shape sh = pick_shape(len_hint);
    if (sh.variant & 4)
        std::snprintf(buf, sizeof(buf), "%s (size classes G/U 4/1 x 4 packets, 4/4, 16/4, 32/4, 64/4)", names[sh.variant & 7]);
    else
        std::snprintf(buf, sizeof(buf), "%s<G=%u,U=%u>%s%s", names[sh.variant & 7], sh.G, sh.U,
                      (sh.variant & 8) ? " all rounds in flight" : (sh.variant & 16) ? " descriptors prefetched" : "",
                      sh.max_blocks ? " grid-capped" : "");
    return buf;
}

const char *rns_build_info(void)
{
    return "rns_checksum abi=1 offload-arch=gfx950 kernels=csum_rows_kernel (packed form: 1 KiB rows per 64-packet "
           "region, owners capture two region prefixes and sum their own end chunk; fill mode), csum_rows_rx_kernel "
           "(packed receive verify: the rows plus each owner's header chunks loaded a group ahead), csum_stream_kernel "
           "(receive verify of ACK-sized arenas: owners load their datagrams whole), csum_strided_rx_kernel (receive "
           "verify of fixed-size slots: quad-coalesced rows), csum_rows_tx_kernel (packed transmit finalize through the "
           "rows), csum_txrows_kernel (transmit-shaped chains: packed payload rows + owner-loaded head fragments; "
           "head-fragment fill; whole finalize of NetBuffer chains with the heads written back from LDS), "
           "csum_strided_tiny_kernel "
           "(fixed-size packets <= 64 B at a fixed stride), csum_mixed_kernel (per-wave size-class sort; verify / fill / "
           "transmit-finalize stash modes), csum_rounds_kernel, csum_batch_kernel, csum_chain_kernel (one pass, "
           "per-fragment fold; head-fragment fill) (v_sad_u16 LE sums, v_dot4 BE sums past 128 KiB, wave64, DPP "
           "reductions)";
}

int rns_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

}  // extern "C"
