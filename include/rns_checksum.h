/*
 * rns_checksum.h — C ABI of the MI355X-native Internet checksum path.
 *
 * Drop-in boundary for jbush001/RustNetworkStack's checksum core
 * (src/stack/util.rs:86-119, 180-207).  The reference binds native code with
 * `#[repr(C)]` structs and `extern "C"` functions returning int
 * (src/stack/netif.rs:24-37, built by build.rs:19-21); this header follows the
 * same convention: plain pointers and sizes, no HIP or torch types, status
 * codes instead of exceptions.  INTEGRATION.md shows the Rust `extern "C"`
 * block and build.rs lines a maintainer would add.
 *
 * Two groups of entry points:
 *
 *  1. Per-packet host calls with the reference's exact signatures and results.
 *     They run on the calling CPU thread (a GPU launch costs microseconds; one
 *     packet costs ~100 ns), are re-entrant, and are what util.rs's four
 *     functions forward to.  Where the reference panics they return a negative
 *     status; the Rust shim turns that back into the same panic.
 *
 *  2. Batch calls that run the hand-written gfx950 kernels over many packets at
 *     once: device-resident (descriptors + arena already in HBM) and
 *     host-resident (pinned staging, overlapped copies).  They never fall back
 *     to the CPU: without a usable GPU they return RNS_E_NODEVICE.
 *
 * Result semantics (both groups, bit-exact with util.rs:88-106): the value is
 * the reference's u32 accumulator — seed + sum of big-endian 16-bit words, an
 * odd final byte counted as (byte << 8), wrapping mod 2^32 like a release
 * build — folded end-around to 16 bits.  RNS_FLAG_COMPLEMENT XORs it with
 * 0xffff, which is what every call site stores or tests (ip.rs:76,158;
 * tcp.rs:848,970; udp.rs:168; icmp.rs:46,71,91,110).
 */
#ifndef RNS_CHECKSUM_H
#define RNS_CHECKSUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNS_ABI_VERSION 1

/* ---- status codes (0 = ok, < 0 = error; never abort) ------------------- */
#define RNS_OK            0
#define RNS_E_INVALID    (-1)  /* bad argument (NULL pointer, bad address length, ...)  */
#define RNS_E_EMPTY      (-2)  /* empty slice: the reference panics (util.rs:92)           */
#define RNS_E_BOUNDS     (-3)  /* a packet descriptor lies outside its arena               */
#define RNS_E_NODEVICE   (-4)  /* no usable gfx950 device / HIP runtime                     */
#define RNS_E_ORDER      (-5)  /* host batch: offsets not ascending                         */
#define RNS_E_TOOLARGE   (-6)  /* host batch: one packet larger than the staging chunk      */
#define RNS_E_IO         (-7)  /* batched I/O: read/write/poll failed (see errno)            */
#define RNS_E_HIP_BASE   (-1000) /* RNS_E_HIP_BASE - hipError_t: HIP runtime error          */

/* ---- flags for batch calls ---------------------------------------------- */
#define RNS_FLAG_COMPLEMENT 0x1u   /* store 0xffff ^ sum (the transmitted / verified value) */
#define RNS_FLAG_CHAIN_RUNS 0x2u   /* rns_csum_chain_dev: fragments are often views of one buffer (see there) */
#define RNS_FLAG_CHAIN_TX_PACKED 0x4u  /* chains: transmit-shaped, payloads packed (rns_csum_chain_fill_dev) */

/* Fragment of a packet, same layout as the reference's `#[repr(C)] struct IOVec
 * { base: *const u8, len: usize }` (netif.rs:24-29). */
typedef struct rns_iovec {
    const uint8_t *base;
    size_t len;
} rns_iovec;

/* IP address, the C form of `enum IPAddr { V4([u8;4]), V6([u8;16]) }`
 * (util.rs:22-26): version is 4 or 6; V4 uses bytes[0..4]. */
typedef struct rns_ipaddr {
    uint32_t version;
    uint8_t bytes[16];
} rns_ipaddr;

/* ========================================================================
 * 1. Per-packet host calls (util.rs)
 * ====================================================================== */

/* util.rs:88 `pub fn compute_ones_comp(in_checksum: u16, slice: &[u8]) -> u16`.
 * Returns the 16-bit sum (>= 0), or RNS_E_EMPTY for len == 0 / RNS_E_INVALID. */
int32_t rns_compute_ones_comp(uint16_t in_checksum, const uint8_t *slice, size_t len);

/* util.rs:108 `pub fn compute_checksum(slice: &[u8]) -> u16` = 0xffff ^ ones_comp(0, slice). */
int32_t rns_compute_checksum(const uint8_t *slice, size_t len);

/* util.rs:112 `pub fn compute_buffer_ones_comp(initial_sum: u16, buffer: &NetBuffer) -> u16`.
 * `frags` are the slices NetBuffer::iter yields (buf.rs:466-487), folded one at
 * a time, so an odd-length non-final fragment is zero-padded like the reference.
 * An empty fragment returns RNS_E_EMPTY (the reference would panic on it). */
int32_t rns_compute_buffer_ones_comp(uint16_t initial_sum, const rns_iovec *frags, size_t nfrags);

/* util.rs:180 `pub fn compute_pseudo_header_checksum(source_ip, dest_ip, length: usize,
 * protocol: u8) -> u16`.  Layout follows dest_ip's version (util.rs:186); a
 * source of the other version is RNS_E_INVALID (the reference panics in copy_to). */
int32_t rns_compute_pseudo_header_checksum(const rns_ipaddr *source_ip, const rns_ipaddr *dest_ip,
                                           uint64_t length, uint8_t protocol);

/* ========================================================================
 * 2. Batch calls (HIP kernels for gfx950)
 * ====================================================================== */

/* What a device entry (every rns_*_dev call below) does with `stream`.
 *   - Every kernel launch of the call is issued on `stream`, and so is everything the call clears first: a
 *     sequence of launches zeroes its counters and clears its tables with a kernel of its own, never with a
 *     memset (a memset node of a captured graph did not repeat its pattern on later replays).
 *   - The call neither synchronises nor reads device memory on the host: counts, ranks and ids that one launch
 *     needs from another stay on the device, and a grid is sized from the by-value arguments alone.
 *   - Everything the call needs from d_work it initialises itself, whatever the workspace held before: poison,
 *     or what another batch of any shape left there.  Nothing is kept in the library between calls (there are
 *     no device globals), so calls on different streams share nothing but the arrays they are given.
 *   - A call, or a chain of calls on one stream (place -> flow update -> ACK build -> plan -> segment; demux ->
 *     send; listen -> connection update -> control build), may therefore be stream-captured once and replayed
 *     over new contents of the same arrays.  What is fixed at capture time is exactly what is passed by value:
 *     the counts and caps, buf_log2, ip_id_base, flags and hints, the local addresses (their bytes are copied
 *     into the launch) and the pointers.  Everything behind a pointer, d_ip_id_add's dword included, is read
 *     when the launch runs.
 * Outside this contract by design: rns_csum_batch_multi_dev (it switches devices and launches on each shard's
 * stream) and the host-resident entries (rns_csum_batch_host, rns_csum_batch_multi_host, rns_io_*), which copy,
 * wait and read back.
 * tests/test_gpu_streams.py holds the pool, TCP and UDP entries to it. */

/* Device-resident batch.  All pointers are device pointers on the current HIP
 * device; `stream` is a hipStream_t (NULL = the null stream).  Packet i is the
 * bytes d_arena[d_off[i] .. d_off[i] + d_len[i]) at any byte alignment; its seed
 * is d_seed[i] (d_seed == NULL => 0).  d_out[i] receives the result.
 * A descriptor outside [0, arena_bytes) gets d_out[i] = 0 and is counted in
 * *d_bad (device u32, optional, not reset by the call).  len == 0 gives the seed
 * (the reference panics).  `len_hint` is the typical packet
 * length in bytes (0 = unknown): it only picks the lanes-per-packet shape.
 * Asynchronous: returns after the launch; errors of the launch itself are
 * returned, never raised. */
int rns_csum_batch_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_off,
                       const uint32_t *d_len, const uint16_t *d_seed, uint16_t *d_out, uint32_t n,
                       uint32_t flags, uint32_t len_hint, uint32_t *d_bad, void *stream);

/* Compact descriptors: as rns_csum_batch_dev (util.rs:88-110 per packet) with
 * 32-bit packet offsets (arenas below 4 GiB), 10 B of descriptors per packet
 * instead of 14.  Same results. */
int rns_csum_batch_dev_off32(const uint8_t *d_arena, uint64_t arena_bytes, const uint32_t *d_off32,
                             const uint32_t *d_len, const uint16_t *d_seed, uint16_t *d_out, uint32_t n,
                             uint32_t flags, uint32_t len_hint, uint32_t *d_bad, void *stream);

/* Packed descriptors: packets lie back to back in index order, packet i+1
 * starting at the first multiple of 2^align_log2 at or after the end of packet i
 * (align_log2 <= 12), as a batched receive packs datagrams into one arena.  Only
 * the lengths travel (d_len16: u16 per packet — an IP datagram's length field is
 * 16 bits) plus d_blk_off[b] = the offset of packet 64*b, one u64 per 64 packets
 * (rns_packed_layout computes them): 2.1 B of descriptors per packet instead of
 * 10 (off32) or 14.  Per packet exactly util.rs:88-110, as rns_csum_batch_dev;
 * a packet outside the arena gets 0 and is counted in *d_bad.  With align_log2 >= 4
 * every batch but one of tiny packets (len_hint <= 112) is streamed as whole 1 KiB
 * rows of its 64-packet blocks, whatever the packet sizes (the rows kernel). */
int rns_csum_batch_packed_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_blk_off,
                              const uint16_t *d_len16, uint32_t align_log2, const uint16_t *d_seed, uint16_t *d_out,
                              uint32_t n, uint32_t flags, uint32_t len_hint, uint32_t *d_bad, void *stream);

/* Host helper for the packed form: given the n lengths, the alignment and the
 * first packet's offset, writes the (n + 63) / 64 block offsets to blk_off and
 * the offset just past the last packet's padded end to *end (the arena size the
 * packing needs).  Optionally (off != NULL) every packet's offset.  CPU only. */
int rns_packed_layout(const uint16_t *len16, uint64_t n, uint32_t align_log2, uint64_t first_off, uint64_t *blk_off,
                      uint64_t *off, uint64_t *end);

/* Same, for packets at a fixed stride (no offset/length arrays to read):
 * packet i = d_arena[first_off + i*stride .. + len).  Offsets that would wrap 64 bits are
 * RNS_E_INVALID (also for rns_rx_verify_strided_dev). */
int rns_csum_batch_strided_dev(const uint8_t *d_arena, uint64_t arena_bytes, uint64_t first_off,
                               uint64_t stride, uint32_t len, const uint16_t *d_seed, uint16_t *d_out,
                               uint32_t n, uint32_t flags, uint32_t *d_bad, void *stream);

/* Fragment chains: util.rs:112 `compute_buffer_ones_comp` for a batch of
 * NetBuffer-style fragment lists (buf.rs:466-487).  Packet i is fragments
 * [d_first[i], d_first[i+1]) of (d_frag_off, d_frag_len) — d_first has n_pkts+1
 * entries; each fragment is folded on its own and the running sum is folded after
 * every fragment, exactly as the reference's loop: an odd-length non-final
 * fragment is zero-padded like the per-fragment call, and the result is exact for
 * ANY fragment count and fragment size (a fragment past 128 KiB wraps the u32
 * accumulator from the running sum, as util.rs:89-99 does in a release build).
 * One pass, one kernel; d_frag_sums is unused (the round-1 two-pass scratch; may
 * be NULL).  A packet whose range is malformed (end < start, end > n_frags) or
 * that has a fragment outside the arena gets 0 and is counted in *d_bad.  An empty
 * fragment contributes nothing (the reference panics on it).
 * RNS_FLAG_CHAIN_RUNS (a hint; results are identical without it): a packet whose
 * <= 4 fragments lie back to back in memory, every one but the last of even length,
 * <= 128 KiB in all, has the same result as that contiguous range (the fragments'
 * words pair identically), so the kernel checks each wave's packets for this and
 * sums a wave whose packets all qualify as contiguous packets.  Set it when the
 * fragments are views of whole receive buffers (c3 as [492, 512, 496]: 287 -> 263 us);
 * without such runs the check costs a descriptor round (shuffled 512-byte buffers:
 * 268 -> 283 us), so it is off by default. */
/* Packets per chain call, at most (both chain entries; the kernel indexes a wave's 64 x 8
 * packets in 32 bits): a larger n_pkts is RNS_E_INVALID. */
#define RNS_CHAIN_MAX_PACKETS (0xFFFFFFFFu - 512u)
int rns_csum_chain_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_frag_off,
                       const uint32_t *d_frag_len, uint32_t n_frags, const uint32_t *d_first,
                       const uint16_t *d_seed, uint16_t *d_out, uint32_t n_pkts, uint32_t flags,
                       uint32_t frag_len_hint, uint16_t *d_frag_sums, uint32_t *d_bad, void *stream);

/* Transmit fill over fragment chains, the shape the reference actually transmits:
 * tcp_output / udp_output / icmp_output_* (tcp.rs:957-973, udp.rs:158-171,
 * icmp.rs:87-112) checksum a NetBuffer whose FIRST fragment is the head fragment
 * alloc_header prepended (buf.rs:262-291, zero-filled, so the field counts as zero:
 * buf.rs:286-288), then set_be16 the result into header_mut() = that fragment.  Packet i
 * = the CSR chain of rns_csum_chain_dev; its field is at byte d_field[i] (NULL =>
 * field_off for every packet: TCP 16, UDP 6, ICMP 2) of fragment d_first[i].  The chain
 * is folded exactly as compute_buffer_ones_comp(d_seed[i], chain) with the field's two
 * bytes counted as zero, and the result (0xffff ^ sum with RNS_FLAG_COMPLEMENT, as every
 * call site stores it; UDP's 0 is stored as is) is stored big-endian into the field.
 * d_out (optional) receives the results.  A packet with no fragments, a malformed range,
 * a fragment outside the arena, or a head fragment too short for its field is left
 * untouched, gets d_out 0 and is counted in *d_bad.  Fragments of different packets
 * must not overlap a field.  RNS_FLAG_CHAIN_RUNS: the hint of rns_csum_chain_dev (the
 * head fragment then starts each run).  Lay the head fragments of consecutive packets
 * back to back in a header region (a batching transmit path's header arena): a wave's
 * 64 field stores then land in a few cache lines instead of 64 scattered ones.
 * RNS_FLAG_CHAIN_TX_PACKED (a hint for this entry and rns_csum_chain_dev; results are
 * identical without it): packets are [a head fragment with (start & 15) + length <= 64,
 * then payload fragments (at most 4) that form a run: back to back, even non-final
 * lengths, <= 65535 bytes], and the payloads of consecutive packets ascend at 16-byte-
 * aligned starts (a packed payload region).  Each 64-packet block's payloads then stream
 * as one region (the rows kernel) while every owner sums its own head; a block that does
 * not have this shape takes an exact per-packet loop (slow; use the hint only for such
 * batches: a batch whose mean fragment count per packet exceeds 5 ignores the hint and
 * runs the chain kernel). */
int rns_csum_chain_fill_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_frag_off,
                            const uint32_t *d_frag_len, uint32_t n_frags, const uint32_t *d_first,
                            const uint16_t *d_seed, const uint16_t *d_field, uint32_t field_off, uint16_t *d_out,
                            uint32_t n_pkts, uint32_t flags, uint32_t frag_len_hint, uint32_t *d_bad, void *stream);

/* Transmit in-place fill (tcp.rs:957-973, udp.rs:158-171, icmp.rs:87-112,
 * ip.rs:158-159): for packet i, sum d_arena[d_off[i] .. + d_len[i]) seeded with
 * d_seed[i], counting the 2-byte checksum field at packet offset d_field[i]
 * (d_field == NULL => field_off for every packet: TCP 16, UDP 6, ICMP 2, IPv4
 * header 10) as zero — the reference zero-fills it (buf.rs:286-288) — and store
 * the result (0xffff ^ sum with RNS_FLAG_COMPLEMENT, as every call site does)
 * big-endian into the field (set_be16).  UDP keeps the reference's behaviour of
 * storing 0 as-is (no RFC 768 0 -> 0xffff).  d_out (optional) also receives the
 * results.  Packets must not overlap.  A packet outside the arena or too short
 * for its field is left untouched, gets d_out 0, and is counted in *d_bad. */
int rns_csum_fill_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_off, const uint32_t *d_len,
                      const uint16_t *d_seed, const uint16_t *d_field, uint32_t field_off, uint16_t *d_out,
                      uint32_t n, uint32_t flags, uint32_t *d_bad, void *stream);

/* Transmit in-place fill of a PACKED transmit arena (the descriptor form of
 * rns_csum_batch_packed_dev: u16 lengths, d_blk_off[b] = offset of packet 64*b,
 * packets back to back at 2^align_log2 boundaries, align_log2 >= 4): per packet exactly
 * what rns_csum_fill_dev does (tcp.rs:957-973, udp.rs:158-171, icmp.rs:87-112,
 * ip.rs:158-159) — the field at d_field[i] (NULL => field_off) counted as zero, the
 * result stored big-endian into it, d_out (optional) and *d_bad as there.  One wave
 * streams each 64-packet block's bytes as whole 1 KiB rows (the rows kernel); the owner
 * of a packet rewrites the 32-byte sector around its field when it lies inside the
 * packet.  len_hint = the typical packet length (kernel depth).  align_log2 < 4 is
 * RNS_E_INVALID. */
int rns_csum_fill_packed_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_blk_off, const uint16_t *d_len16,
                             uint32_t align_log2, const uint16_t *d_seed, const uint16_t *d_field, uint32_t field_off,
                             uint16_t *d_out, uint32_t n, uint32_t flags, uint32_t len_hint, uint32_t *d_bad,
                             void *stream);

/* Receive verify (§8f row 1): for each received IP datagram
 * d_arena[d_off[i] .. + d_len[i]), the checks the stack applies before handing it
 * to the transport layer — ip_input_v4 header checksum (ip.rs:76-80), fragment
 * drop (ip.rs:84-87), protocol dispatch (ip.rs:123-131), TCP validate_checksum
 * with the pseudo-header built from the source address and the LOCAL address
 * (tcp.rs:838-850), ICMPv4 (icmp.rs:46-50), ICMPv6 (icmp.rs:62-75); UDP is not
 * verified by the stack (udp.rs:126-148).  As in the reference, the L4 length is
 * the buffer length minus the IP header (the total-length field is not used).
 * One fused pass over the datagram bytes.  d_status[i] gets RNS_RX_* bits;
 * d_l4_sum (optional) the complemented L4 sum. */
#define RNS_RX_IP_OK          0x01u  /* IPv4 header checksum verifies (always set for IPv6) */
#define RNS_RX_L4_OK          0x02u  /* TCP / ICMPv4 / ICMPv6 checksum verifies */
#define RNS_RX_L4_UNCHECKED   0x04u  /* UDP: the stack does not verify it */
#define RNS_RX_FRAGMENT       0x08u  /* IPv4 fragment: the stack drops it */
#define RNS_RX_UNKNOWN_PROTO  0x10u  /* protocol the stack drops */
#define RNS_RX_ACCEPT         0x40u  /* the stack would deliver it to its transport handler */
#define RNS_RX_MALFORMED      0x80u  /* bad version / too short: the reference drops or panics */
int rns_rx_verify_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_off, const uint32_t *d_len,
                      uint32_t n, const uint8_t *local_ipv4, const uint8_t *local_ipv6, uint8_t *d_status,
                      uint16_t *d_l4_sum, void *stream);

/* Receive verify of a PACKED receive arena (the descriptor form of
 * rns_csum_batch_packed_dev: u16 lengths, d_blk_off[b] = offset of datagram 64*b),
 * with datagrams starting on 16-byte boundaries (align_log2 >= 4; 2048-byte receive
 * slots qualify): per datagram exactly the checks and status bits of rns_rx_verify_dev
 * (ip.rs:65-131, tcp.rs:838-850, icmp.rs:44-75).  One wave streams each 64-datagram
 * block's bytes as whole 1 KiB rows whatever the datagram sizes (the stream kernel);
 * a block of ACK-sized datagrams (all <= 64 B) is read by its owners directly, which
 * keeps them at the plain checksum's rate.  align_log2 < 4 is RNS_E_INVALID. */
int rns_rx_verify_packed_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_blk_off,
                             const uint16_t *d_len16, uint32_t align_log2, uint32_t n, const uint8_t *local_ipv4,
                             const uint8_t *local_ipv6, uint8_t *d_status, uint16_t *d_l4_sum, void *stream);

/* Receive verify of datagrams at a FIXED STRIDE (a receive ring of fixed-size slots:
 * the reference's 2048-byte MRU buffers, netif.rs:66, or 64-byte ACK slots): datagram i
 * = d_arena[first_off + i * stride .. + d_len16[i]); per datagram exactly the checks and
 * status bits of rns_rx_verify_dev (ip.rs:65-131, tcp.rs:838-850, icmp.rs:44-75).  No
 * offsets travel and there is no per-block scan: with 16-byte-aligned slots every lane
 * loads its datagram's first 64 bytes beside its length, so an ACK-sized datagram costs
 * one memory round; longer datagrams are summed by a whole wave each.  Any stride and
 * alignment is accepted (datagrams may even overlap: nothing is written to the arena). */
int rns_rx_verify_strided_dev(const uint8_t *d_arena, uint64_t arena_bytes, uint64_t first_off, uint64_t stride,
                              const uint16_t *d_len16, uint32_t n, const uint8_t *local_ipv4, const uint8_t *local_ipv6,
                              uint8_t *d_status, uint16_t *d_l4_sum, void *stream);

/* Receive verify of NetBuffer FRAGMENT CHAINS, as the reference holds a received datagram
 * (recv_packet, netif.rs:65-83: new_prealloc(2048) = four 512-byte pool fragments, trim_tail):
 * datagram i = fragments [d_first[i], d_first[i+1]) of (d_frag_off, d_frag_len), the CSR form
 * of rns_csum_chain_dev, anywhere in the arena at any byte alignment.  Nothing is written to
 * the arena.  The RNS_RX_* bits mean what they mean for rns_rx_verify_dev, decided as the
 * reference decides them on a NetBuffer; with len0 = the first fragment's length and T = the
 * sum of all fragment lengths:
 *   - header() is the FIRST fragment only (ip.rs:39, 69, 115): the version is header[0] >> 4;
 *     IPv4: hdr = IHL*4, RNS_RX_MALFORMED when hdr == 0, len0 < 16 or hdr > len0, the header
 *     checksum over header[..hdr] and the fields [6..8], [9], [12..16] from that fragment;
 *     IPv6: hdr = 40, RNS_RX_MALFORMED when len0 < 24 (header[8..24]) or T < 40 (trim_head asserts);
 *   - the L4 segment is the chain after trim_head(hdr) (buf.rs:294-329): whole fragments go while
 *     their length does not exceed what remains to trim, then the next fragment's start advances
 *     (a head fragment of exactly hdr bytes disappears; an IPv6 header may run over several short
 *     fragments); its length is T - hdr, which the TCP / ICMPv6 pseudo-header carries;
 *   - the L4 value is compute_buffer_ones_comp(seed, segment) ^ 0xffff (util.rs:112-119): folded
 *     after every fragment, each fragment paired from its own start, an odd-length fragment
 *     zero-padded as util.rs:97-99 pads it, a fragment past 128 KiB wrapping the u32 accumulator
 *     as util.rs:89-99 does; an empty segment yields the seed;
 *   - RNS_RX_MALFORMED (d_l4_sum 0) also for a malformed range (first[i] > first[i+1] or
 *     first[i+1] > n_frags), a datagram without fragments (header() asserts), any fragment
 *     outside the arena, and len0 == 0 (header[0] panics).
 * An EMPTY fragment after the first adds nothing; the reference would panic on it (util.rs:92),
 * so parity is unpinned there, as for the other len == 0 cases of this header.  A one-fragment
 * chain gives exactly what rns_rx_verify_dev gives for (off, len).
 * One pass: the fragments stream through the chain kernel's class pass, the owner lane parses
 * its head fragment's first bytes and takes the header's words out of that fragment's sum.  An
 * IPv6 header that runs past its first fragment, or a fragment past 128 KiB, sends its datagram
 * through an exact per-datagram loop (same results, slower).  n_pkts == 0 is RNS_OK; a NULL
 * d_arena / d_first / d_status / local address, NULL fragment arrays with n_frags > 0, or
 * n_pkts > RNS_CHAIN_MAX_PACKETS is RNS_E_INVALID, all before the device is touched. */
int rns_rx_verify_chain_dev(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_frag_off,
                            const uint32_t *d_frag_len, uint32_t n_frags, const uint32_t *d_first, uint32_t n_pkts,
                            const uint8_t *local_ipv4, const uint8_t *local_ipv6, uint8_t *d_status,
                            uint16_t *d_l4_sum /* optional */, void *stream);

/* Receive verify of datagrams held in fixed-size POOL BUFFERS (recv_packet's chains):
 * buffers of 2^buf_log2 bytes (6 <= buf_log2 <= 15; the reference's FRAGMENT_SIZE is 2^9),
 * buffer k = d_pool[k << buf_log2 .. ).  Datagram i has length d_len16[i] and occupies
 * nf_i = ceil(len_i / 2^buf_log2) buffers, all full but the last; their indices are
 * d_buf_idx[first_i .. first_i + nf_i), where first_i = d_blk_first[i / 64] + the sum of nf_k over
 * the datagrams k of i's 64-datagram block before i.  (The blocks' entries are independent of each
 * other, as the block offsets of rns_csum_batch_packed_dev are.)  Descriptors: 2 B per datagram,
 * 4 B per buffer, 4 B per 64 datagrams — 14 B for a 1500-byte datagram in 512-byte buffers
 * against the CSR form's 40 B.
 * The form is defined by the CSR chain it expands to: fragment j of datagram i at offset
 * (uint64_t)d_buf_idx[first_i + j] << buf_log2, of 2^buf_log2 bytes, the last one of the remainder.
 * d_status[i] and d_l4_sum[i] are exactly what rns_rx_verify_chain_dev gives for that chain on the
 * same pool.  It follows that
 *   - a datagram with d_len16[i] == 0 has no fragments: RNS_RX_MALFORMED, d_l4_sum 0 (header()
 *     asserts in the reference, so parity is unpinned there, as for the other len == 0 cases);
 *   - a fragment whose bytes end past pool_bytes makes its datagram, and that one only,
 *     RNS_RX_MALFORMED;
 *   - first_i + nf_i > n_frags is RNS_RX_MALFORMED;
 *   - two datagrams may name the same buffer: nothing is written to the pool.
 * Because every buffer starts 16-byte aligned and holds at least 64 bytes, the header lies in the
 * first buffer at an aligned start and every fragment before the last has even length: the kernel
 * has neither the chain kernel's unaligned head path nor its exact per-datagram loop.
 * n_pkts == 0 is RNS_OK; buf_log2 outside 6..15, a NULL d_pool / d_blk_first / d_len16 / d_status /
 * local address, a NULL d_buf_idx with n_frags > 0, n_pkts > RNS_CHAIN_MAX_PACKETS or a d_pool that
 * is not 16-byte aligned is RNS_E_INVALID, all before the device is touched. */
int rns_rx_verify_pool_dev(const uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2,
                           const uint32_t *d_buf_idx, uint32_t n_frags,
                           const uint32_t *d_blk_first,   /* (n_pkts + 63) / 64 entries */
                           const uint16_t *d_len16, uint32_t n_pkts,
                           const uint8_t *local_ipv4, const uint8_t *local_ipv6,
                           uint8_t *d_status, uint16_t *d_l4_sum /* optional */, void *stream);

/* Host helper for the pool form (CPU only): from the n lengths, blk_first ((n + 63) / 64 entries),
 * optionally first[0..n] (the CSR index of the expanded chains) and *n_frags.  RNS_E_INVALID if the
 * fragment total does not fit 32 bits or buf_log2 is outside 6..15. */
int rns_rx_pool_layout(const uint16_t *len16, uint64_t n, uint32_t buf_log2,
                       uint32_t *blk_first, uint32_t *first /* optional, n + 1 */, uint64_t *n_frags);

/* TCP receive placement over pool buffers: what tcp_input does after validate_checksum, and
 * tcp_read's copy, on the device — the receive twin of rns_tx_segment_dev.  For the pool form
 * above (same pool, same descriptors) every accepted TCP segment is decoded (tcp.rs:549-574), its
 * flow looked up by PORT_MAP's key (tcp.rs:577-578) in a table the host built, and its payload
 * copied to its place in that flow's contiguous receive window: window start + (seq - next expected
 * seq).  The place comes from the sequence number, so segments may arrive in any order within a
 * batch and no datagram depends on another.  After the call the host holds 24 bytes per datagram
 * (d_meta) to drive the control plane, and the bytes tcp_read would deliver (tcp.rs:230-246,
 * buf.rs:424-441) lie contiguous in d_stream.
 * The form is defined by what it expands to:
 *   Status: d_status[i] and d_l4_sum[i] are exactly what rns_rx_verify_pool_dev gives for the same
 *     pool and descriptors.
 *   Decode: with T = d_len16[i], ip_hdr as the verify parses it (IHL * 4, or 40) and L = T - ip_hdr,
 *     datagram i is decoded (RNS_PLACE_TCP) iff its status has RNS_RX_ACCEPT, its protocol is 6,
 *     L >= 20 and 20 <= tcp_hdr = 4 * (byte 12 >> 4) <= L.  Then sport, dport, seq, ack and window
 *     are the header's big-endian fields, flags = byte 13 and pay_len = L - tcp_hdr.  Everything
 *     else has place 0, flow RNS_RX_NO_FLOW and every other field 0.  (The reference panics on
 *     header[0..20] / header[20..header_length] / trim_head for the short cases: parity is unpinned
 *     there.)  Options are not parsed: parse_options loops forever on a zero option length, and a
 *     SYN's options are the host's business.
 *   Lookup: the key is the source address (family from the IP version), sport and dport;
 *     RNS_PLACE_FLOW is set and flow is the key's index iff the key is in the table.  The listen
 *     socket fallback and the RST reply (tcp.rs:579-615) stay on the host, which sees RNS_PLACE_TCP
 *     without RNS_PLACE_FLOW.  With n_flows == 0 every datagram is unmatched and d_tbl is not read.
 *   Placement: with f = flow and d = (seq - d_next_seq[f]) mod 2^32, the payload is placed
 *     (RNS_PLACE_DONE) iff the segment is decoded with a flow, pay_len > 0, neither SYN nor RST is
 *     set, d < d_win_len[f], pay_len <= d_win_len[f] - d and d_win_off[f] + d_win_len[f] <=
 *     stream_bytes (computed without overflow).  Then d_stream[d_win_off[f] + d + k] = byte
 *     ip_hdr + tcp_hdr + k of the datagram for k in [0, pay_len): with o = ip_hdr + tcp_hdr + k, the
 *     byte at offset o & (B - 1) of buffer d_buf_idx[first_i + (o >> buf_log2)], B = 2^buf_log2.  A
 *     segment with a flow and payload, no SYN / RST, that fails the window test gets
 *     RNS_PLACE_OUTSIDE (stale, straddling next_seq, past the window's end, or a window past
 *     stream_bytes) and nothing is written for it.  No byte of d_stream outside the placed ranges
 *     is written and nothing is ever written to the pool.  Windows of different flows must not
 *     overlap.  Two placed segments of one batch may overlap within a window: each such byte then
 *     holds one of the two values, which TCP makes equal.  The per-flow arrays are read-only;
 *     advancing next_seq and sliding the window is the host's job.
 * Whatever the descriptors, the table and the per-flow arrays hold, nothing outside the pool,
 * tbl_bytes and the arrays is read and nothing outside d_stream[0 .. stream_bytes) is written.
 * Descriptors: the pool form's, plus 16 B per flow and the table (32 B per slot); 24 B of d_meta
 * come back per datagram.
 * n_pkts == 0 is RNS_OK; buf_log2 outside 7..15 (60 + 60 header bytes must lie in the first buffer:
 * the verify's 6 is too small), a NULL d_pool / d_blk_first / d_len16 / d_status / d_meta /
 * d_next_seq / d_win_off / d_win_len / d_stream / local address, a NULL d_tbl with n_flows > 0, a
 * NULL d_buf_idx with n_frags > 0, a d_pool that is not 16-byte aligned, a d_meta or d_tbl that is
 * not 4-byte aligned, tbl_bytes below what rns_rx_flow_table_build asks for n_flows, or n_pkts >
 * RNS_CHAIN_MAX_PACKETS is RNS_E_INVALID, all before the device is touched. */
#define RNS_RX_NO_FLOW 0xffffffffu
typedef struct rns_rx_flow_key {      /* PORT_MAP's key, tcp.rs:578: the REMOTE address and port, the local port */
    uint8_t ip[16];                   /* family 4: ip[0..4], ip[4..16] zero; family 6: all 16 */
    uint16_t sport, dport;            /* host byte order: the segment's source port, its destination port */
    uint8_t family, pad[3];           /* 4 or 6; pad zero */
} rns_rx_flow_key;                    /* 24 bytes */
typedef struct rns_rx_tcp_meta {      /* 24 bytes; fields in host byte order */
    uint32_t flow;                    /* index into the per-flow arrays, RNS_RX_NO_FLOW if none */
    uint32_t seq, ack;
    uint16_t sport, dport, window, pay_len;
    uint8_t flags, ip_hdr, tcp_hdr, place;
} rns_rx_tcp_meta;
#define RNS_PLACE_TCP     0x01u  /* decoded: the other fields are valid */
#define RNS_PLACE_FLOW    0x02u  /* its key is in the table */
#define RNS_PLACE_DONE    0x04u  /* its payload was copied into its flow's window */
#define RNS_PLACE_OUTSIDE 0x08u  /* it has a flow and payload, but the window does not take it */
int rns_rx_tcp_place_pool_dev(const uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2,
                              const uint32_t *d_buf_idx, uint32_t n_frags,
                              const uint32_t *d_blk_first,   /* (n_pkts + 63) / 64 entries */
                              const uint16_t *d_len16, uint32_t n_pkts,
                              const uint8_t *local_ipv4, const uint8_t *local_ipv6,
                              const uint8_t *d_tbl, uint64_t tbl_bytes,   /* rns_rx_flow_table_build's, on the device */
                              const uint32_t *d_next_seq,    /* n_flows: the next expected sequence number */
                              const uint64_t *d_win_off,     /* n_flows: the window's start in d_stream */
                              const uint32_t *d_win_len,     /* n_flows: its bytes */
                              uint32_t n_flows,
                              uint8_t *d_stream, uint64_t stream_bytes,
                              uint8_t *d_status, uint16_t *d_l4_sum /* optional */, rns_rx_tcp_meta *d_meta,
                              void *stream);

/* Host helper for the placement's flow table (CPU only): *need_bytes = the table's size for n_flows
 * keys, and, when tbl is non-NULL, the table itself, key f mapped to flow index f.  Only this
 * function writes a table and only the kernel reads it; copy the bytes to the device as they are.
 * Layout: 32-byte slots, their count the smallest power of two >= 2 * n_flows and >= 64, an empty
 * slot all zero, a taken one six little-endian dwords of key (ip[0..16) as bytes, sport | dport <<
 * 16, family), the flow index and 1.  A key's probe starts at slot h & (slots - 1), h = 0x9e3779b9
 * then per key dword w: h = (h ^ w) * 0x85ebca6b mod 2^32, h ^= h >> 15, and goes on linearly
 * (wrapping) to the first empty slot.  Whatever bytes a table holds, the kernel's probe ends within
 * the slot count and a stored flow >= n_flows is no match.  RNS_E_INVALID for a duplicate key, a
 * family other than 4 or 6, non-zero padding or non-zero ip[4..16] with family 4, a NULL need_bytes,
 * a NULL keys with n_flows > 0, or tbl_bytes below the need (the table's contents are then
 * unspecified; nothing past tbl_bytes is ever written). */
int rns_rx_flow_table_build(const rns_rx_flow_key *keys, uint32_t n_flows,
                            uint8_t *tbl /* NULL: size only */, uint64_t tbl_bytes, uint64_t *need_bytes);

/* ICMP echo responder over pool buffers: icmp_input_v4 / icmp_input_v6 (icmp.rs:44-85) with their
 * icmp_output_* and ip_output_* on the device.  For a receive batch in the pool form above, every echo
 * request becomes a finished echo reply in a transmit pool, described by the compact descriptors
 * rns_tx_fill_pool_dev and rns_io_send_batch_pool take; its buffers are drawn from a free list on the
 * device and its IPv4 id is numbered as NEXT_PACKET_ID would number it.  The host touches no datagram.
 * Both pools have buffers of 2^buf_log2 bytes, B below.
 * The form is defined by what it expands to:
 *   Status: d_status[i] and d_l4_sum[i] are exactly what rns_rx_verify_pool_dev gives for the same
 *     pool and descriptors.
 *   Request: with T = d_len16[i] and h the IP header length as the verify parses it (IHL * 4, or 40),
 *     datagram i is a request (RNS_ECHO_REQUEST) iff its status has RNS_RX_ACCEPT, T - h >= 4, and it
 *     is IPv4 with protocol 1 and L4 byte 0 == 8, or IPv6 with next header 58 and L4 byte 0 == 128.
 *     The code byte is not looked at.  Everything else has d_echo[i] == 0: bad checksums, echo
 *     replies, other ICMP types, protocol 1 over IPv6 or 58 over IPv4, TCP, UDP, IPv4 fragments,
 *     malformed datagrams.  (If the verify accepted the crossed-protocol cases, the reference would
 *     answer them through icmp_input_v4 with an IPv6 address; and it panics in trim_head(4) for
 *     T - h < 4.  Parity is unpinned for both.)
 *   Allocation: request i needs nf_i = 1 + ceil(pay_i / B) buffers, pay_i = T - h - 4.  With R_i and
 *     F_i the inclusive counts of requests and of their buffers up to i in batch order, it is answered
 *     iff R_i <= reply_cap and F_i <= n_free; both counts are monotone, so the answered requests are a
 *     prefix of the requests.  The others get RNS_ECHO_NOBUF and nothing is written for them: the host
 *     answers those.  Reply r = R_i - 1 takes d_free[F_i - nf_i .. F_i), head buffer first, so the reply
 *     descriptors' buf_idx IS d_free[0 .. d_count[1]) itself (d_free is read-only), d_tx_blk_first[r / 64]
 *     is the number of buffers before reply 64 * (r / 64), d_tx_head_len8[r] is 24 or 44, d_tx_pay_len16[r]
 *     = pay_i, d_tx_src[r] = i, and d_count = {replies, buffers, IPv4 replies}.  Entries of the
 *     descriptor arrays at and past d_count[0] (for d_tx_blk_first: of blocks without a reply) are not
 *     written.  (The buffers are counted as payload buffers + requests, the payload buffers in 32 bits:
 *     always exact up to 2^24 datagrams; a batch whose requests hold 2^32 payload buffers or more is
 *     outside the domain — still nothing outside the arrays and the pools is read or written.)
 *   Bytes: the head is the LAST 24 / 44 bytes of the head buffer, as alloc_header(4) and then
 *     alloc_header(20 / 40) leave it: IPv4 45 00, total length 24 + pay (mod 2^16: an accepted header
 *     shorter than 20 bytes can pass it), id = (ip_id_base + *d_ip_id_add + the IPv4 replies before it)
 *     mod 2^16, flags/offset 0, TTL 64, protocol 1, the header checksum, source = the LOCAL address (not
 *     the request's destination), destination = the requester; IPv6 60 00 00 00, payload length 4 + pay,
 *     next header 58, hop limit 64, local address, requester, and no id taken.  Then type 0 / 129, code 0
 *     (alloc_header zeroes: the request's code is not echoed) and the checksum
 *     compute_buffer_ones_comp(seed, packet) ^ 0xffff, seed 0 (IPv4) or the pseudo-header of (local,
 *     requester, 4 + pay, 58).  IPv4 options of the request are dropped.  Payload byte k is byte
 *     o = h + 4 + k of the request — offset o & (B - 1) of buffer d_buf_idx[first_i + (o >> buf_log2)] —
 *     and goes to offset k & (B - 1) of the reply's buffer 1 + (k >> buf_log2): whole buffers from offset
 *     0 and a last one with the remainder (append_from_buffer), none for pay == 0.  The stored bytes equal
 *     those rns_tx_fill_pool_dev produces from the same heads with zeroed checksum fields.
 *     Only a reply's own buffers are written: the head bytes, the payload bytes, and at most the bytes
 *     from the payload's end up to the next 16-byte boundary of its last buffer (unspecified values: the
 *     buffer is the reply's alone and a sender reads pay bytes).  Every other byte of the transmit pool,
 *     the whole receive pool and every input array stay as they were.  A reply with any buffer index >=
 *     tx_pool_bytes >> buf_log2 is counted and described, but gets d_tx_head_len8[r] = 0 (malformed to
 *     rns_tx_fill_pool_dev and the sender) and RNS_ECHO_REQUEST | RNS_ECHO_BADBUF without
 *     RNS_ECHO_BUILT, and nothing is written for it.  The two pools may be the same memory when no
 *     d_free buffer is named by d_buf_idx.
 * The launches after the verify: one that classifies, two one-workgroup scans, and one that copies each
 * payload once — summing what it copies — and writes the heads, both checksums filled.
 * n_pkts == 0 is RNS_OK with d_count zeroed.  buf_log2 outside 8..15, a NULL d_rx_pool / d_blk_first /
 * d_len16 / d_status / d_echo / d_count / d_tx_pool / d_work / local address, a NULL d_buf_idx with
 * n_frags > 0, a NULL d_free with n_free > 0, a pool that is not 16-byte aligned, a d_work that is not
 * 8-byte aligned, work_bytes below rns_rx_icmp_echo_work's answer, or n_pkts > RNS_CHAIN_MAX_PACKETS is
 * RNS_E_INVALID, all before the device is touched.  d_tx_blk_first / d_tx_head_len8 / d_tx_pay_len16 may
 * be NULL iff reply_cap == 0; d_tx_src, d_l4_sum and d_ip_id_add are optional. */
#define RNS_ECHO_REQUEST 0x01u  /* an echo request the stack would answer */
#define RNS_ECHO_BUILT   0x02u  /* its reply was built and is described in the tx descriptors */
#define RNS_ECHO_NOBUF   0x04u  /* a request past reply_cap or past the free list: the host answers it */
#define RNS_ECHO_BADBUF  0x08u  /* a buffer it drew from d_free lies outside the tx pool: nothing written */
int rns_rx_icmp_echo_pool_dev(const uint8_t *d_rx_pool, uint64_t rx_pool_bytes, uint32_t buf_log2,
                              const uint32_t *d_buf_idx, uint32_t n_frags,
                              const uint32_t *d_blk_first,   /* (n_pkts + 63) / 64 entries */
                              const uint16_t *d_len16, uint32_t n_pkts,
                              const uint8_t *local_ipv4, const uint8_t *local_ipv6,
                              uint8_t *d_tx_pool, uint64_t tx_pool_bytes,   /* the same buf_log2 */
                              const uint32_t *d_free, uint32_t n_free,      /* free tx buffers, taken in order */
                              uint32_t reply_cap,
                              uint16_t ip_id_base, const uint32_t *d_ip_id_add /* optional device dword, added to the base */,
                              uint32_t *d_tx_blk_first /* (reply_cap + 63) / 64 */, uint8_t *d_tx_head_len8,
                              uint16_t *d_tx_pay_len16, uint32_t *d_tx_src /* optional, reply_cap: the request's index */,
                              uint32_t *d_count /* 3 dwords: replies, buffers taken, IPv4 ids taken */,
                              uint8_t *d_status, uint16_t *d_l4_sum /* optional */, uint8_t *d_echo /* n_pkts */,
                              void *d_work, uint64_t work_bytes, void *stream);

/* The responder's workspace in bytes for n_pkts datagrams (CPU only): non-zero and monotone in n_pkts.
 * RNS_E_INVALID for a NULL bytes or n_pkts > RNS_CHAIN_MAX_PACKETS. */
int rns_rx_icmp_echo_work(uint32_t n_pkts, uint64_t *bytes);

/* UDP receive demux over pool buffers: udp_input (udp.rs:126-148) on the device — the UDP twin of
 * rns_rx_tcp_place_pool_dev.  For a receive batch in the pool form above, every accepted UDP datagram
 * whose destination port has a socket becomes one entry of that socket's receive_queue: a 32-byte record
 * (source address, source port, length) and its payload, copied to a 16-byte-aligned place in d_data.  A
 * socket's entries are contiguous, in arrival order, so the bytes successive udp_recv calls (udp.rs:75-98)
 * hand out lie in order on the device, and the host reads one dword per socket and 32 B per delivered
 * datagram instead of touching every datagram.
 * The form is defined by what it expands to:
 *   Status: d_status[i] and d_l4_sum[i] are exactly what rns_rx_verify_pool_dev gives for the same pool
 *     and descriptors.
 *   Decode: with T = d_len16[i] and h the IP header length as the verify parses it (IHL * 4, or 40),
 *     datagram i is a UDP datagram (RNS_UDP_DGRAM) iff its status has RNS_RX_ACCEPT, its protocol (IPv4
 *     byte 9, IPv6 byte 6) is 17 and T - h >= 8.  sport and dport are the header's big-endian fields and
 *     the payload is bytes [h + 8, T) of the datagram: byte o at offset o & (B - 1) of buffer
 *     d_buf_idx[first_i + (o >> buf_log2)], B = 2^buf_log2.  The UDP length field and the UDP checksum are
 *     not looked at: the reference reads neither.  Everything else has d_udp[i] == 0.  (For T - h < 8 the
 *     reference panics in header[2..4] / trim_head(8): parity is unpinned there.)
 *   Lookup: s = d_port_tbl[dport]; RNS_UDP_SOCK is set iff s < n_socks.  Anything else takes the "No
 *     socket listening" path: dropped, no record.  With n_socks == 0 every UDP datagram is RNS_UDP_DGRAM
 *     without a socket and d_port_tbl is not read.  Sockets past RNS_UDP_MAX_SOCKS stay on the host and
 *     show as unbound here.
 *   Queues: socket s's entries are the datagrams with RNS_UDP_SOCK and socket s in ascending i, the order
 *     push_back would have met them, and the queues are laid out socket-major: position(i) = (entries of
 *     sockets < s) + (entries of s before i).  off16 follows the same order, each payload taking
 *     ceil(len / 16) units of 16 bytes: every payload starts 16-byte aligned, and a zero-length datagram
 *     is an entry with no units (the reference queues it, and udp_recv returns 0 for it).
 *     d_q_first[s] = the position of s's first entry, d_q_first[n_socks] = all entries, and d_count =
 *     {entries, units}, both counted before any cut.  (The units are counted in 32 bits, which the bound on
 *     n_frags below makes exact unless blocks of d_blk_first share entries of d_buf_idx; such a batch is
 *     outside the domain — still nothing outside the arrays is read or written.)
 *   Cut: entry i is RNS_UDP_QUEUED iff position < rec_cap and 16 * (off16 + units) <= data_bytes.
 *     Otherwise it is RNS_UDP_NOROOM: no record is written, no byte copied, d_pos[i] = 0xffffffff, and the
 *     host queues it.  With rec_cap >= n_pkts and data_bytes >= n_frags << buf_log2 nothing is ever cut.
 *   Bytes: a queued entry's record goes to d_rec[position] (flags = d_udp[i]) and its payload to
 *     d_data[16 * off16 ..).  At most the bytes from the payload's end to the next 16-byte boundary of its
 *     own range may also be written, with unspecified values.  No other byte of d_data or d_rec is written;
 *     d_pos[i] is the position of a queued entry and 0xffffffff for every other datagram.  The pool and
 *     every input stay as they were.  The same inputs give the same bytes on every run.
 * Whatever the descriptors and the table hold, nothing outside the pool, the table's 65536 entries and the
 * arrays is read, and nothing outside d_data[0 .. data_bytes), d_rec[0 .. rec_cap) and the per-datagram
 * and per-socket outputs is written.
 * The launches after the verify: one that classifies and counts per (socket, tile of 512 datagrams), the
 * three of a prefix sum over those counts, and one that ranks, writes the records and copies each payload
 * once.  No atomic decides an output.
 * n_pkts == 0 is RNS_OK with d_count zeroed and d_q_first[0 .. n_socks] zero.  n_socks >
 * RNS_UDP_MAX_SOCKS, buf_log2 outside 7..15 (60 + 8 header bytes must lie in the first buffer), a NULL
 * d_pool / d_blk_first / d_len16 / d_status / d_udp / d_q_first / d_count / d_work / local address, a NULL
 * d_buf_idx with n_frags > 0, a NULL d_port_tbl with n_socks > 0, a NULL d_data with data_bytes > 0, a NULL
 * d_rec with rec_cap > 0, a d_pool, d_data, d_rec or d_work that is not 16-byte aligned, work_bytes below
 * rns_rx_udp_demux_work's answer, n_pkts > RNS_CHAIN_MAX_PACKETS, or (uint64_t)n_frags << buf_log2 >= 2^36
 * (so that the unit counts fit 32 bits) is RNS_E_INVALID, all before the device is touched. */
#define RNS_UDP_MAX_SOCKS 1024u
#define RNS_UDP_NO_SOCK   0xffffu
#define RNS_UDP_DGRAM   0x01u  /* decoded as UDP: udp_input would be called on it */
#define RNS_UDP_SOCK    0x02u  /* its destination port has a socket */
#define RNS_UDP_QUEUED  0x04u  /* its record is written and its payload copied */
#define RNS_UDP_NOROOM  0x08u  /* it has a socket, but rec_cap or data_bytes does not take it: the host queues it */
typedef struct rns_udp_rec {          /* 32 bytes: one receive_queue entry */
    uint8_t  ip[16];                  /* source address: family 4 in ip[0..4], rest zero */
    uint32_t src;                     /* the datagram's index in the batch */
    uint32_t off16;                   /* payload start in d_data, in units of 16 bytes */
    uint16_t sport, len;              /* host byte order; len = payload bytes (may be 0) */
    uint8_t  family, flags, pad[2];   /* 4 / 6; flags = d_udp[src]; pad zero */
} rns_udp_rec;
int rns_rx_udp_demux_pool_dev(const uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2,
                              const uint32_t *d_buf_idx, uint32_t n_frags,
                              const uint32_t *d_blk_first,   /* (n_pkts + 63) / 64 entries */
                              const uint16_t *d_len16, uint32_t n_pkts,
                              const uint8_t *local_ipv4, const uint8_t *local_ipv6,
                              const uint16_t *d_port_tbl /* 65536 entries: rns_rx_udp_port_table_build's */,
                              uint32_t n_socks,
                              uint8_t *d_data, uint64_t data_bytes,
                              rns_udp_rec *d_rec, uint32_t rec_cap,
                              uint32_t *d_q_first /* n_socks + 1 */, uint32_t *d_count /* 2: records, 16-byte units */,
                              uint8_t *d_status, uint16_t *d_l4_sum /* optional */, uint8_t *d_udp /* n_pkts */,
                              uint32_t *d_pos /* optional, n_pkts: record position or 0xffffffff */,
                              void *d_work, uint64_t work_bytes, void *stream);

/* The demux's workspace in bytes for n_pkts datagrams and n_socks sockets (CPU only): non-zero, monotone
 * in both, at most 64 MiB for 2^20 datagrams and 1024 sockets.  RNS_E_INVALID for a NULL bytes, n_pkts >
 * RNS_CHAIN_MAX_PACKETS or n_socks > RNS_UDP_MAX_SOCKS. */
int rns_rx_udp_demux_work(uint32_t n_pkts, uint32_t n_socks, uint64_t *bytes);

/* Host helper for the demux's port table (CPU only), PORT_MAP as an array: all 65536 entries of tbl are
 * set to RNS_UDP_NO_SOCK, then tbl[ports[s]] = s (ports in host byte order).  Copy the table to the device
 * as it is.  RNS_E_INVALID for a duplicate port (udp_open's "Port already in use"; the table's contents are
 * then unspecified), n_socks > RNS_UDP_MAX_SOCKS, a NULL tbl, or a NULL ports with n_socks > 0. */
int rns_rx_udp_port_table_build(const uint16_t *ports, uint32_t n_socks, uint16_t *tbl /* 65536 */);

/* UDP send build over pool buffers: udp_send -> udp_output -> ip_output_v4 / ip_output_v6 (udp.rs:101-114 and
 * 150-173, ip.rs:133-177) for a batch of sends on the device — the UDP twin of the echo responder's build step.
 * Every send becomes a finished datagram in a transmit pool, described by the compact descriptors
 * rns_tx_fill_pool_dev and rns_io_send_batch_pool take; its buffers are drawn from a free list on the device and
 * its IPv4 id is numbered as NEXT_PACKET_ID would number it.  It reads the demux's records as they are, so
 * receive -> demux -> send -> sendmmsg is one stream of launches (the reference's udp_echo.rs: udp_recv, then
 * udp_send back to the sender) and the host touches no datagram.  Buffers have 2^buf_log2 bytes, B below.
 * The form is defined by what it expands to:
 *   A record read as a send: rns_udp_rec is taken unchanged.  The send goes TO ip (family 4: ip[0..4], family 6:
 *     all 16), TO port sport, with the len bytes at d_data[16 * off16 ..).  src and pad are not read.  The demux's
 *     output is therefore an echo server's input with no transformation; a host that builds sends of its own
 *     fills the same struct with flags = RNS_UDP_QUEUED.
 *   Which records are sends: record k < n_recs is a send (RNS_UDPTX_SEND) iff k < d_q_first[n_socks] — read on
 *     the device: the host need not read it back and may pass n_recs = rec_cap — its flags have RNS_UDP_QUEUED,
 *     its family is 4 or 6, and 16 * off16 + len <= data_bytes (computed in 64 bits).  Every other record has
 *     d_send[k] == 0 and takes no buffer and no id.  The demux writes no record for an RNS_UDP_NOROOM entry, so
 *     a d_rec that was zeroed before a cut demux is safe to pass whole: the unwritten records lack
 *     RNS_UDP_QUEUED.
 *   Source port: d_sock_port[s], s the socket whose range [d_q_first[s], d_q_first[s + 1]) holds k — the demux's
 *     socket-major layout; a host caller groups its sends by socket, which is how udp_send is called anyway.
 *     (s is the last socket with d_q_first[s] <= k, socket 0 if there is none.)  A table that is not
 *     non-decreasing is outside the domain: which socket a record gets is then unspecified — still nothing
 *     outside the arrays is read or written.  n_socks is 1 .. RNS_UDP_MAX_SOCKS.
 *   Allocation (the echo responder's rule): send k needs nf_k = 1 + ceil(len_k / B) buffers.  With R_k and F_k
 *     the inclusive counts of sends and of their buffers up to k in record order, it is built iff R_k <= send_cap
 *     and F_k <= n_free; both counts are monotone, so the built sends are a prefix of the sends.  The others get
 *     RNS_UDPTX_NOBUF and nothing is written for them: the host sends those.  Datagram r = R_k - 1 takes
 *     d_free[F_k - nf_k .. F_k), head buffer first, so the descriptors' buf_idx IS d_free[0 .. d_count[1]) itself
 *     (d_free is read-only), d_tx_blk_first[r / 64] is the number of buffers before datagram 64 * (r / 64),
 *     d_tx_head_len8[r] is 28 or 48, d_tx_pay_len16[r] = len_k, d_tx_src[r] = k, and d_count = {datagrams,
 *     buffers, IPv4 datagrams}.  Entries of the descriptor arrays at and past d_count[0] (for d_tx_blk_first: of
 *     blocks without a datagram) are not written.  (The buffers are counted as payload buffers + sends, the
 *     payload buffers in 32 bits: always exact up to 2^24 records; a batch whose sends hold 2^32 payload buffers
 *     or more is outside the domain — still nothing outside the arrays and the pool is read or written.)
 *   Bytes: the datagram is laid out as append_from_slice, then alloc_header(8), then alloc_header(20 / 40) leave
 *     it: the head is the LAST 28 / 48 bytes of the head buffer, and payload byte j is at offset j & (B - 1) of
 *     buffer 1 + (j >> buf_log2): whole buffers from offset 0 and a last one with the remainder, none for
 *     len == 0.  IPv4: 45 00, total length (28 + len) mod 2^16, id = (ip_id_base + *d_ip_id_add + the IPv4 sends
 *     before it) mod 2^16 in record order, flags/offset 0, TTL 64, protocol 17, the header checksum, source =
 *     the local address, then the destination.  IPv6: 60 00 00 00, payload length (8 + len) mod 2^16, next
 *     header 17, hop limit 64, the local address, the destination, and no id taken.  UDP: source port,
 *     destination port, length (8 + len) mod 2^16, and the checksum compute_buffer_ones_comp(pseudo(local,
 *     destination, that length, 17), packet) ^ 0xffff; a computed 0 is stored as 0, as the reference stores it.
 *     The mod-2^16 lengths are the reference's `as u16` and are pinned, not corrected.  The stored bytes equal
 *     those rns_tx_fill_pool_dev produces from the same heads with zeroed checksum fields.
 *     Only a datagram's own buffers are written: the head bytes, the payload bytes, and at most the bytes from
 *     the payload's end up to the next 16-byte boundary of its last buffer (unspecified values: the buffer is
 *     the datagram's alone and a sender reads len bytes).  Every other byte of the transmit pool, d_data, d_rec
 *     and every input array stay as they were.  A datagram with any buffer index >= tx_pool_bytes >> buf_log2
 *     is counted and described, but gets d_tx_head_len8[r] = 0 (malformed to rns_tx_fill_pool_dev and the
 *     sender) and RNS_UDPTX_SEND | RNS_UDPTX_BADBUF without RNS_UDPTX_BUILT, and nothing is written for it.
 *     The same inputs give the same bytes on every run.
 * The launches: one that classifies, two one-workgroup scans, and one that copies each payload once — summing
 * what it copies — and writes the heads, both checksums filled.  No atomic decides an output.
 * n_recs == 0 is RNS_OK with d_count zeroed.  buf_log2 outside 8..15, n_socks == 0 or > RNS_UDP_MAX_SOCKS, a
 * NULL d_data / d_rec / d_q_first / d_sock_port / d_tx_pool / d_count / d_send / d_work / local address, a NULL
 * d_free with n_free > 0, a d_data, d_rec or d_tx_pool that is not 16-byte aligned, a d_work that is not 8-byte
 * aligned, work_bytes below rns_tx_udp_send_work's answer, or n_recs > RNS_CHAIN_MAX_PACKETS is RNS_E_INVALID,
 * all before the device is touched.  d_tx_blk_first / d_tx_head_len8 / d_tx_pay_len16 may be NULL iff
 * send_cap == 0; d_tx_src and d_ip_id_add are optional. */
#define RNS_UDPTX_SEND   0x01u  /* a well-formed send: udp_send would be called for it */
#define RNS_UDPTX_BUILT  0x02u  /* its datagram is built and described in the tx descriptors */
#define RNS_UDPTX_NOBUF  0x04u  /* past send_cap or past the free list: the host sends it */
#define RNS_UDPTX_BADBUF 0x08u  /* a buffer it drew lies outside the tx pool: nothing written */
int rns_tx_udp_send_pool_dev(const uint8_t *d_data, uint64_t data_bytes,
                             const rns_udp_rec *d_rec, uint32_t n_recs,
                             const uint32_t *d_q_first /* n_socks + 1 */,
                             const uint16_t *d_sock_port /* n_socks, host byte order */, uint32_t n_socks,
                             const uint8_t *local_ipv4, const uint8_t *local_ipv6,
                             uint8_t *d_tx_pool, uint64_t tx_pool_bytes, uint32_t buf_log2,
                             const uint32_t *d_free, uint32_t n_free,      /* free tx buffers, taken in order */
                             uint32_t send_cap,
                             uint16_t ip_id_base, const uint32_t *d_ip_id_add /* optional device dword, added to the base */,
                             uint32_t *d_tx_blk_first /* (send_cap + 63) / 64 */, uint8_t *d_tx_head_len8,
                             uint16_t *d_tx_pay_len16, uint32_t *d_tx_src /* optional, send_cap: the record's index */,
                             uint32_t *d_count /* 3 dwords: datagrams, buffers taken, IPv4 ids taken */,
                             uint8_t *d_send /* n_recs */,
                             void *d_work, uint64_t work_bytes, void *stream);

/* The send build's workspace in bytes for n_recs records (CPU only): non-zero and monotone in n_recs.
 * RNS_E_INVALID for a NULL bytes or n_recs > RNS_CHAIN_MAX_PACKETS. */
int rns_tx_udp_send_work(uint32_t n_recs, uint64_t *bytes);

/* TCP flow update: the rest of tcp_input for an Established socket (tcp.rs:642-740) on the device,
 * over the placement's d_meta as it is — the advance of receive_next_seq and the reassembler's
 * next_sequence, the delayed-ACK count and its immediate ACKs, the ACK-field check that trims the
 * retransmit queue, the send-window update.  This is header prediction: for every flow f < n_flows
 * its segments of the batch are walked in batch order, the first one that is not the fast path's
 * stops the flow, and the host takes over from there with the state of the consumed prefix.
 *   Which datagrams: flow f's list is the datagrams i with d_meta[i].place & RNS_PLACE_FLOW and
 *     d_meta[i].flow == f < n_flows, in ascending i (the order tcp_input would have met them in).
 *     Every other datagram gets an all-zero d_seg record.
 *   Stops, tested before each segment in this order (a flow without segments never stops); the
 *   segment that stops the flow and all its later ones get zero d_seg records, d_res[f].stop is its
 *   datagram index and d_res[f].why the reason:
 *     RNS_STOP_MANY     the list has more than RNS_FLOW_MAX_SEGS entries (nothing is consumed, stop =
 *                       the flow's first datagram).  The reference advertises at most 65535 bytes and
 *                       no window scale, so a flow has fewer than 64 KiB in flight; the cap lets a
 *                       flow's list fit on chip.
 *     RNS_STOP_STATE    state != RNS_TCP_ESTABLISHED at the start of the batch, or n_pend > pend_cap
 *                       on input (nothing is consumed).
 *     RNS_STOP_FLAGS    SYN, RST or FIN is set: the RST hack (tcp.rs:635) and the state machine
 *                       (tcp.rs:742-835) are the host's.
 *     RNS_STOP_OPTIONS  tcp_hdr != 20: parse_options is the host's, as in the placement (it loops for
 *                       ever on a zero option length: parity is unpinned there).  With 20 bytes
 *                       tcp.rs:622-625 is a no-op.
 *     RNS_STOP_OUTSIDE  place & RNS_PLACE_OUTSIDE: the bytes are not in the window.
 *     RNS_STOP_PEND     pay_len > 0, seq != rcv_nxt and n_pend == pend_cap: no room to remember it.
 *   Step of a consumed segment (act has RNS_SEG_CONSUMED), exactly tcp.rs:642-740 with state ==
 *   Established, seq_gt / seq_lt / seq_le as util.rs:155-166:
 *     Data (tcp.rs:642-687), when pay_len > 0 (the placement has then set RNS_PLACE_DONE):
 *       rcv_max = wrapping_max(rcv_max, seq + pay_len) (util.rs:172);
 *       got = TCPReassembler::add_packet over (seq, pay_len) (tcp.rs:488-516) with the Vec's own
 *         semantics: seq != rcv_nxt appends (seq, pay_len) at the end of the pending list and got =
 *         0; else got = pay_len, rcv_nxt += pay_len and the list is rescanned from i = 0: an entry
 *         with seq_gt(the ARRIVING seq, entry.seq) is removed, an entry with entry.seq == rcv_nxt is
 *         removed, rcv_nxt += its length, got += its length and the scan restarts at 0; a removal
 *         moves the tail down one place;
 *       rq_len += got, readable += got; delayed_acks += 1 (mod 2^16); if it is then >= 5
 *       (MAX_DELAYED_ACKS): delayed_acks = 0, ack_timer = 0, act |= RNS_SEG_ACK with ack_num =
 *       rcv_nxt and window = (0xffff - (rq_len & 0xffff)) & 0xffff (send_packet, tcp.rs:403-417; the
 *       FIN + 1 never applies in Established), n_acks += 1; otherwise, if ack_timer == 0: ack_timer =
 *       1 and act |= RNS_SEG_TIMER.  (With rq_len > 0xffff the reference computes MAX_RECEIVE_WINDOW
 *       - len as u16, which panics in a debug build and wraps in a release one: parity is unpinned
 *       there, and so it is for the panicking decodes inherited from the placement.)
 *     ACK field (tcp.rs:698-740), when flags & 0x10: if seq_lt(snd_una, ack) && seq_le(ack, snd_nxt):
 *       acked += ack - snd_una, snd_una = ack.  Then, with the new snd_una, if seq_le(snd_una, ack)
 *       && seq_le(ack, snd_nxt) && (seq_lt(snd_wl1, seq) || (snd_wl1 == seq && seq_le(snd_wl2,
 *       ack))): snd_wnd = window, snd_wl1 = seq, snd_wl2 = ack, events |= RNS_EV_WND.
 *   Timers are the host's: it derives them from consumed > 0 (the response timer's cancel),
 *   ack_timer (arm or cancel the delayed-ACK timer) and acked (cancel the retransmit timer when the
 *   queue empties).
 * d_flow_out[f], d_res[f] and every datagram's d_seg record are written on every call; d_pend_out
 * holds flow f's list in entries [f * pend_cap, f * pend_cap + n_pend), the entries past n_pend are
 * unspecified.  A flow stopped at its first segment has d_flow_out[f] == d_flow_in[f] bytewise.  The
 * in and out arrays must not overlap, and d_meta must not change during the call.  Whatever meta,
 * state and pending lists hold (n_pend > pend_cap, flow >= n_flows, any place bits), nothing outside
 * the argument arrays is read or written.  The call allocates nothing: d_work is the caller's,
 * work_bytes at least what rns_rx_tcp_flow_update_work gives for (n_pkts, n_flows); its contents
 * before and after the call mean nothing.
 * n_pkts == 0 still writes every flow's out record (a copy) and a zero result; n_flows == 0 writes
 * zero d_seg records.  A NULL d_meta / d_seg with n_pkts > 0, a NULL d_flow_in / d_flow_out / d_res
 * with n_flows > 0, a NULL d_pend_in / d_pend_out with n_flows > 0 and pend_cap > 0, a NULL d_work
 * with n_pkts + n_flows > 0, any of these arrays not 4-byte aligned (d_work: 8-byte), work_bytes below the need,
 * n_pkts > RNS_CHAIN_MAX_PACKETS or n_flows >= 2^31 is RNS_E_INVALID, all before the device is
 * touched. */
#define RNS_TCP_ESTABLISHED 1u
#define RNS_FLOW_MAX_SEGS   1024u
typedef struct rns_tcp_flow {   /* 40 bytes, host byte order */
    uint32_t rcv_nxt;           /* reassembler.next_sequence (tcp.rs:110) */
    uint32_t rcv_max;           /* receive_next_seq */
    uint32_t snd_una, snd_nxt, snd_wnd, snd_wl1, snd_wl2; /* send_unacked, send_next_seq, send_window, send_last_win_seq / _ack */
    uint32_t rq_len;            /* receive_queue.len() */
    uint32_t n_pend;            /* out_of_order.len(), <= pend_cap */
    uint16_t delayed_acks;      /* num_delayed_acks */
    uint8_t  state;             /* RNS_TCP_ESTABLISHED; anything else is not the fast path's */
    uint8_t  ack_timer;         /* 1: delayed_ack_timer_id != -1 */
} rns_tcp_flow;
/* d_pend: pend_cap (seq, len) u32 pairs per flow, the reassembler's out_of_order Vec IN ITS ORDER;
 * pend_cap == 0 allows NULL d_pend_*. */
typedef struct rns_rx_tcp_seg { uint32_t ack_num; uint16_t window; uint8_t act, pad; } rns_rx_tcp_seg; /* 8 bytes */
#define RNS_SEG_CONSUMED 1u   /* the fast path processed it */
#define RNS_SEG_ACK      2u   /* an immediate ACK was sent after it: ack_num / window are that ACK's */
#define RNS_SEG_TIMER    4u   /* it started the delayed-ACK timer */
typedef struct rns_tcp_flow_res {   /* 24 bytes */
    uint32_t n_segs;      /* the flow's datagrams in the batch */
    uint32_t consumed;    /* how many of them, from the front, were processed */
    uint32_t stop;        /* datagram index of the first one not processed, 0xffffffff if none */
    uint32_t readable;    /* bytes appended to receive_queue (sum of add_packet's returned lengths) */
    uint32_t acked;       /* bytes trimmed from the retransmit queue */
    uint16_t n_acks;      /* immediate ACKs sent */
    uint8_t events;       /* RNS_EV_WND */
    uint8_t why;          /* RNS_STOP_* */
} rns_tcp_flow_res;
#define RNS_EV_WND       1u   /* the send window was updated */
#define RNS_STOP_NONE    0u
#define RNS_STOP_MANY    1u
#define RNS_STOP_STATE   2u
#define RNS_STOP_FLAGS   3u
#define RNS_STOP_OPTIONS 4u
#define RNS_STOP_OUTSIDE 5u
#define RNS_STOP_PEND    6u
int rns_rx_tcp_flow_update_dev(const rns_rx_tcp_meta *d_meta, uint32_t n_pkts, uint32_t n_flows,
                               const rns_tcp_flow *d_flow_in, const uint32_t *d_pend_in, uint32_t pend_cap,
                               rns_tcp_flow *d_flow_out, uint32_t *d_pend_out,
                               rns_rx_tcp_seg *d_seg,       /* n_pkts */
                               rns_tcp_flow_res *d_res,     /* n_flows */
                               void *d_work, uint64_t work_bytes, void *stream);

/* The workspace of rns_rx_tcp_flow_update_dev (CPU only): *bytes for n_pkts datagrams and n_flows
 * flows, monotone in both; it also covers rns_tx_ack_build_dev for the same n_pkts.  A NULL bytes,
 * n_pkts > RNS_CHAIN_MAX_PACKETS or n_flows >= 2^31 is RNS_E_INVALID. */
int rns_rx_tcp_flow_update_work(uint32_t n_pkts, uint32_t n_flows, uint64_t *bytes);

/* ACK build: the pure ACKs the update decided on, as send_packet(NetBuffer::new(), FLAG_ACK) ->
 * tcp_output (tcp.rs:938-976) -> ip_output (ip.rs:140-177) builds them, finalized, in batch order.
 * ACK k belongs to the k-th datagram i in ascending i with d_seg[i].act & RNS_SEG_ACK and
 * f = d_meta[i].flow < n_flows (an ACK flag on a datagram whose flow >= n_flows is ignored).  Its
 * head, hl = d_head_len8[f] bytes at d_out + 64 * k, is its flow's template (d_tmpl + f *
 * tmpl_stride, as in rns_tx_segment_dev) verbatim except
 *   TCP at the IP header's end: [4..8] = d_flow[f].snd_nxt, [8..12] = d_seg[i].ack_num, [12] = 0x50,
 *                         [13] = 0x10, [14..16] = d_seg[i].window, [16..18] = the checksum;
 *   IPv4 (hl == 40):      [2..4] = 40, [4..6] = ip_id_base + (the IPv4 ACKs among ACKs 0..k-1) mod
 *                         2^16 — NEXT_PACKET_ID.fetch_add runs in ip_output_v4 only and the reference
 *                         answers in batch order, so these are its ids —, [10..12] = the header
 *                         checksum;
 *   IPv6 (hl == 60):      [4..6] = 20.
 * The result is what rns_tx_fill_dev stores for that head as a datagram without payload.  Bytes
 * [hl, 64) of a slot are not written.  d_ack_src[k] = i and d_ack_len8[k] = hl, so the slots go out
 * through rns_io_send_batch(off = 64 * k, len = d_ack_len8[k]).  A malformed template — hl neither
 * 40 nor 60, hl > tmpl_stride, hl == 40 without t[0] == 0x45 and t[9] == 6, hl == 60 without
 * t[0] >> 4 == 6 and t[6] == 6, or a TCP data offset t[iphdr + 12] >> 4 other than 5 — keeps its
 * slot and (an ACK is an IPv4 one, and takes an id, iff hl == 40) its id, gets d_ack_len8[k] = 0 and
 * no byte of its slot is written.  ACKs at and past ack_cap are counted but not written, neither slot
 * nor d_ack_src nor d_ack_len8.  d_n_acks[0] = the ACKs, d_n_acks[1] = the IPv4 ones, always
 * written.  ack_cap == 0 allows NULL d_out / d_ack_src / d_ack_len8: the call counts only.  d_work
 * as above (the update's workspace serves, once the update is done).
 * A NULL d_n_acks; with n_pkts > 0 a NULL d_meta / d_seg / d_work, work_bytes below the need or,
 * with n_flows > 0, a NULL d_flow / d_tmpl / d_head_len8 or tmpl_stride == 0; with ack_cap > 0 a
 * NULL d_out / d_ack_src / d_ack_len8; a d_meta / d_seg / d_flow / d_out / d_ack_src / d_n_acks that
 * is not 4-byte aligned or a d_work that is not 8-byte aligned; or n_pkts > RNS_CHAIN_MAX_PACKETS is RNS_E_INVALID, all before
 * the device is touched. */
int rns_tx_ack_build_dev(const rns_rx_tcp_meta *d_meta, const rns_rx_tcp_seg *d_seg, uint32_t n_pkts,
                         const rns_tcp_flow *d_flow, uint32_t n_flows,
                         const uint8_t *d_tmpl, uint32_t tmpl_stride, const uint8_t *d_head_len8,
                         uint16_t ip_id_base, void *d_work, uint64_t work_bytes,
                         uint8_t *d_out, uint32_t ack_cap, uint32_t *d_ack_src, uint8_t *d_ack_len8,
                         uint32_t *d_n_acks /* 2 */, void *stream);

/* TCP listen responder over pool buffers: tcp_input's branch for a segment whose key is not in PORT_MAP
 * (tcp.rs:579-615) with handle_new_connection (tcp.rs:894-936), send_packet, tcp_output and ip_output on
 * the device.  It takes over the branch rns_rx_tcp_place_pool_dev leaves to the host (RNS_PLACE_TCP without
 * RNS_PLACE_FLOW): it reads the placement's d_meta as it is, over the same pool and descriptors, and builds
 * the RST|ACK of every stray segment, the SYN|ACK of every new connection and the new socket's state, the
 * replies in 64-byte slots as rns_tx_ack_build_dev leaves its ACKs.  The verify is not run again and there
 * is no d_status: a decoded meta record says the datagram was accepted.  Every rule is a line of the
 * reference, restated for a batch processed in index order.
 * The form is defined by what it expands to:
 *   Unmatched: datagram i is unmatched (RNS_CONN_UNMATCHED) iff d_meta[i].place has RNS_PLACE_TCP and not
 *     RNS_PLACE_FLOW.  Everything else has d_conn[i] == 0.  Its key (rns_rx_flow_key) is the source
 *     address read from its first pool buffer — bytes 12..16 (IPv4) or 8..24 (IPv6), the family from the
 *     version nibble —, d_meta[i].sport and d_meta[i].dport.  What d_meta claims is checked again before a
 *     byte of the pool is read, as the consumers of a verified batch do: the datagram's fragments inside
 *     d_buf_idx, its first buffer inside the pool, T = d_len16[i] >= 16, the version 4 or 6, ip_hdr the
 *     header length the first buffer gives (IHL * 4, or 40) and >= 20, 20 <= tcp_hdr <= 60 a multiple of
 *     4, ip_hdr + tcp_hdr <= T.  A record that fails (the placement writes none) is no segment: d_conn[i]
 *     == 0.
 *   Candidate: an unmatched datagram is a candidate iff flags & 0x02 (SYN) and d_listen[dport] names a
 *     listener: an entry < n_listen.  d_listen is the table rns_rx_udp_port_table_build writes, over the
 *     listening ports.  No other flag is looked at: SYN|ACK, SYN|RST and SYN|FIN to a listening port all
 *     open a connection in the reference, and a payload on the SYN is ignored.
 *   First of its key: let s(key) be the smallest index among the batch's candidates with that key (the
 *     reference inserts the new socket into PORT_MAP there, tcp.rs:611).  An unmatched datagram i is
 *       i == s(key): a new connection, RNS_CONN_SYN if its options parse (below), else RNS_CONN_HOST: no
 *         reply, no id, no accept record; the host's.  It still owns its key.
 *       i > s(key): RNS_CONN_LATER, whatever became of datagram s (RNS_CONN_NOBUF or RNS_CONN_HOST too):
 *         the reference would find the socket s created, so a duplicate SYN or the handshake's third
 *         segment gets no RST.  The host replays it against the accept record.  No reply, no id.
 *       otherwise (no candidate of its key at or before it): RNS_CONN_RST, a segment that itself
 *         carries RST and a SYN to a port nobody listens on included.
 *   Replies: reply k belongs to the k-th datagram i, in ascending i, with RNS_CONN_SYN or RNS_CONN_RST.
 *     Its head goes to d_out + 64 * k, d_rep_src[k] = i and d_rep_len8[k] = its length, so the slots go
 *     out through rns_io_send_batch(off = 64 * k, len).  Bytes past the length in a slot are not written.
 *     IPv4 replies take the id ip_id_base + *d_ip_id_add (0 without it) + (the IPv4 replies among
 *     replies 0..k-1) mod 2^16; IPv6 replies take none.
 *   Head bytes (tcp_output -> ip_output_v4 / ip_output_v6):
 *     IPv4: 45 00, the total length, the id, 00 00, TTL 64, protocol 6, the header checksum, source = the
 *       local address, destination = the segment's source.
 *     IPv6: 60 00 00 00, the payload length, next header 6, hop limit 64, the local address, the
 *       segment's source.
 *     TCP: source port = the segment's dport, destination port = its sport, urgent pointer 0, the
 *       checksum over the pseudo-header of (local, remote, TCP length, 6), and
 *                      RST (tcp.rs:582-595)            SYN-ACK (send_packet, tcp.rs:402-447)
 *         length       40 (IPv4) / 60 (IPv6)           44 / 64
 *         seq          1                               d_iss[a], a = its rank among the accepts
 *         ack          d_meta[i].seq + 1 mod 2^32      the same
 *         offset byte  0x50                            0x60
 *         flags        0x14                            0x12
 *         window       0                               0xffff
 *         options      none                            02 04 05 dc
 *     The RST's ack does not add the payload length.  The stored bytes equal what rns_tx_fill_dev
 *     produces for the same head as a datagram without payload and with zeroed checksum fields.
 *   Accept record: accept a is the a-th RNS_CONN_SYN datagram in ascending i.  d_accept[a] holds key, src
 *     = i, listener = d_listen[dport], mss (below) and flow as handle_new_connection leaves the socket:
 *     state = RNS_TCP_SYN_RECEIVED, rcv_nxt = rcv_max = seq + 1, snd_nxt = d_iss[a], snd_una = seq (the
 *     reference stores the PEER's sequence number there, tcp.rs:917; not corrected), snd_wl1 = seq,
 *     snd_wl2 = d_meta[i].ack, snd_wnd = d_meta[i].window, every other field 0.  The reference draws
 *     the ISS from rand::random; here the host supplies it, so the same inputs give the same bytes on
 *     every run.
 *   Options: parse_options (tcp.rs:856-892) over the header bytes [20, tcp_hdr) of the first buffer
 *     (buf_log2 >= 7 keeps them there): type 0 ends the walk, type 1 advances by 1, any other type reads
 *     its length byte; type 2 reads the big-endian u16 at +2 as mss, whatever the length byte says, the
 *     last such option wins; the offset then advances by the length.  mss is 0 without the option.
 *     RNS_CONN_HOST covers the inputs on which the reference does not return: a length byte of 0 (it loops
 *     for ever), an option type whose length byte lies past the options' end (it panics), and type 2 with
 *     fewer than 4 bytes left (it panics).  The walk is bounded by the 40 option bytes.
 *   Caps: a reply at or past reply_cap is counted, gets RNS_CONN_NOBUF without RNS_CONN_BUILT, and nothing
 *     is written for it, the accept record of a SYN included: the host answers it.  Its key stays opened.
 *     d_count = (replies, IPv4 replies, accepts), each counted as if reply_cap were unbounded, always
 *     written; with d_count[0] <= reply_cap everything is written, otherwise replies 0 .. reply_cap - 1
 *     and the accepts of the SYNs among them, which are a prefix of the accepts (d_conn says which).  An
 *     accept's rank is never above its reply's, so reply_cap entries of d_accept and d_iss suffice.
 *     reply_cap == 0 allows NULL d_out / d_rep_src / d_rep_len8 / d_accept / d_iss: the call counts and
 *     classifies only.
 * No byte is written outside d_out[0 .. 64 * reply_cap), the first min(count, cap) entries of the reply
 * and accept arrays, d_count, d_conn and d_work; the pool, d_meta and d_listen are read-only.  Whatever
 * meta, descriptors and table hold, nothing outside the arguments is read or written.  The keys of a batch
 * meet in an open-addressing table in d_work through integer atomics; only a key's minimum candidate
 * index is read back, which no order of the atomics changes.  The call allocates nothing: d_work is
 * the caller's, work_bytes at least what rns_rx_tcp_listen_work gives for n_pkts (2^20 datagrams: 28
 * MiB); its contents before and after the call mean nothing.
 * Unpinned: a segment from 0.0.0.0 port 0 (the reference finds the listen socket itself under that key;
 * here it is a source like any other); d_meta[i].seq + 1 for 0xffffffff (the reference's seq_num + 1
 * overflows: a panic in a debug build, a wrap in a release one; here it wraps); the panicking decodes
 * inherited from the placement.  The reference parses the options of every segment before the lookup;
 * here only a first SYN's are walked.
 * n_pkts == 0 is RNS_OK with d_count zeroed.  A NULL d_pool / d_blk_first / d_len16 / d_meta / d_count /
 * d_conn / d_work / local address, a NULL d_buf_idx with n_frags > 0, a NULL d_listen with n_listen > 0, a
 * NULL d_out / d_rep_src / d_rep_len8 / d_accept / d_iss with reply_cap > 0, buf_log2 outside 7..15, a
 * d_pool that is not 16-byte aligned, a d_meta / d_accept / d_out / d_count / d_rep_src / d_iss /
 * d_ip_id_add that is not 4-byte aligned, a d_work that is not 8-byte aligned, n_listen >
 * RNS_UDP_MAX_SOCKS, work_bytes below the need or n_pkts > RNS_CHAIN_MAX_PACKETS is RNS_E_INVALID, all
 * before the device is touched. */
#define RNS_TCP_SYN_RECEIVED 2u           /* rns_tcp_flow.state of an accepted connection */
#define RNS_CONN_UNMATCHED 0x01u  /* decoded TCP (RNS_PLACE_TCP) without RNS_PLACE_FLOW: tcp.rs:579's branch */
#define RNS_CONN_SYN       0x02u  /* SYN to a listening port, the first of its key in the batch: a new connection */
#define RNS_CONN_LATER     0x04u  /* an earlier SYN of this batch opened its key: the new socket's, the host's; no reply */
#define RNS_CONN_RST       0x08u  /* answered with RST|ACK */
#define RNS_CONN_BUILT     0x10u  /* its reply (and, for a SYN, its accept record) is written */
#define RNS_CONN_NOBUF     0x20u  /* a reply at or past reply_cap: counted, nothing written, the host answers */
#define RNS_CONN_HOST      0x40u  /* a first SYN whose options the device does not parse: the host's; no reply */
typedef struct rns_tcp_accept {   /* 72 bytes */
    rns_rx_flow_key key;          /* what handle_new_connection inserts into PORT_MAP */
    rns_tcp_flow    flow;         /* the new socket's state after handle_new_connection */
    uint32_t        src;          /* the SYN's datagram index */
    uint16_t        listener;     /* the listen table's entry for its destination port */
    uint16_t        mss;          /* parse_options' max_segment_size, 0 without the option */
} rns_tcp_accept;
int rns_rx_tcp_listen_pool_dev(const uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2,
                               const uint32_t *d_buf_idx, uint32_t n_frags,
                               const uint32_t *d_blk_first,   /* (n_pkts + 63) / 64 entries */
                               const uint16_t *d_len16, uint32_t n_pkts,
                               const uint8_t *local_ipv4, const uint8_t *local_ipv6,
                               const rns_rx_tcp_meta *d_meta,          /* the placement's, as it is */
                               const uint16_t *d_listen /* 65536 */, uint32_t n_listen,
                               const uint32_t *d_iss,                  /* reply_cap: accept a takes d_iss[a] */
                               uint16_t ip_id_base, const uint32_t *d_ip_id_add /* optional */,
                               uint8_t *d_out /* 64 * reply_cap */, uint32_t reply_cap,
                               uint32_t *d_rep_src, uint8_t *d_rep_len8,   /* reply_cap each */
                               rns_tcp_accept *d_accept,                   /* reply_cap */
                               uint32_t *d_count /* 3: replies, IPv4 replies, accepts */,
                               uint8_t *d_conn /* n_pkts */,
                               void *d_work, uint64_t work_bytes, void *stream);

/* The workspace of rns_rx_tcp_listen_pool_dev (CPU only): *bytes for n_pkts datagrams, monotone in it.  A
 * NULL bytes or n_pkts > RNS_CHAIN_MAX_PACKETS is RNS_E_INVALID. */
int rns_rx_tcp_listen_work(uint32_t n_pkts, uint64_t *bytes);

/* TCP connection update: tcp_input for an existing socket in any state the device takes (tcp.rs:622-835)
 * — the RST hack, the data branch of a socket that is not Established, the ACK field and the state
 * machine — per flow in batch order.  It is rns_rx_tcp_flow_update_dev with a wider step: the arguments
 * d_meta, d_flow_in / d_flow_out, d_pend_in / d_pend_out, pend_cap, d_res and d_work, the membership rule
 * (RNS_PLACE_FLOW and flow < n_flows, ascending datagram index), the overlap and alignment rules (d_ctl:
 * 4-byte aligned), the behaviour for n_pkts == 0 and n_flows == 0, the argument errors and the guarantee
 * that nothing outside the arguments is touched are that entry's, with rns_tcp_ctl *d_ctl (n_pkts
 * records, all written on every call) in place of d_seg.  A flow record of rns_rx_tcp_listen_pool_dev's
 * accept (RNS_TCP_SYN_RECEIVED) goes in as it is, so accept -> handshake -> request -> close is one
 * stream of launches.
 *   Records: a datagram that is no member gets an all-zero record; so do the segment that stops a flow
 *     and every later segment of that flow.  A consumed segment's record has flow = its flow, act with
 *     RNS_CTL_CONSUMED and, with RNS_CTL_SEND, the segment send_packet built at that moment: seq (the
 *     flow's snd_nxt THEN: a SynReceived socket that gets data on its third segment ACKs it before the
 *     + 1 of tcp.rs:771), ack_num, window, flags; without RNS_CTL_SEND these four are 0.
 *   Stops, tested before each segment in this order:
 *     RNS_STOP_MANY     as in the flow update.
 *     RNS_STOP_STATE    n_pend > pend_cap on input, or the flow's current state is RNS_TCP_SYN_SENT,
 *                       RNS_TCP_LISTEN or above 10.
 *     RNS_STOP_OPTIONS  tcp_hdr != 20 (tcp.rs:622-625 needs parse_options).
 *     (RST set: no further stop; the segment is consumed by step A whatever else it carries.)
 *     RNS_STOP_FLAGS    SYN set and pay_len > 0: the reference would queue that payload, the placement
 *                       does not place a SYN's.  A SYN without payload is no stop: the reference never
 *                       looks at SYN on an existing socket.
 *     RNS_STOP_OUTSIDE, RNS_STOP_PEND  as in the flow update.
 *     RNS_STOP_TWICE    pay_len > 0 with FIN in state FIN_WAIT2, or in FIN_WAIT1 unless ACK is set and
 *                       ack == snd_nxt + 1: the reference sends the data branch's ACK and then the
 *                       arm's, and a record holds one send.
 *   Step of a consumed segment; st = the state before it, and the state changes only in A and D:
 *     A. RST (tcp.rs:635-640): state = CLOSED, act = CONSUMED | RESET | STATE, nothing else of the
 *        segment is processed: its payload is dropped and its sequence number not checked.  Later
 *        segments of the flow go on against the Closed socket, as the reference's would.
 *     B. Data (tcp.rs:642-696), pay_len > 0: rcv_max, add_packet over the pending list, rq_len and
 *        readable exactly as in the flow update.  st == ESTABLISHED: the flow update's delayed-ACK
 *        branch, where FIN also forces the immediate ACK (tcp.rs:656); RNS_CTL_ACK_TIMER is
 *        RNS_SEG_TIMER.  Every other state: ack_timer = 0, delayed_acks untouched, and a send.
 *        A send is send_packet(FLAG_ACK) (tcp.rs:402-447): RNS_CTL_SEND, flags = 0x10, seq = snd_nxt as
 *        it is now, ack_num = rcv_nxt, + 1 (wrapping) iff the state at the send is FIN_WAIT1, FIN_WAIT2,
 *        CLOSING or CLOSE_WAIT and rcv_max == rcv_nxt (tcp.rs:408-417), window as in the flow update,
 *        n_acks += 1.
 *     C. ACK field (tcp.rs:698-740), when flags & 0x10 and st is neither CLOSED nor TIME_WAIT: the
 *        flow update's block unchanged.
 *     D. The arms (tcp.rs:742-835):
 *          SYN_RECEIVED  ACK: state ESTABLISHED, snd_nxt += 1, snd_una = ack (unconditional).
 *          ESTABLISHED   FIN: state CLOSE_WAIT, no send.
 *          LAST_ACK      ACK (any number): state CLOSED.
 *          FIN_WAIT1     ACK, FIN and ack == snd_nxt + 1: state TIME_WAIT, RNS_CTL_TIMEWAIT;
 *                        else FIN: state CLOSING, then a send (the + 1 rule sees CLOSING), RNS_CTL_RESP_TIMER;
 *                        else ACK and ack == snd_nxt + 1: state FIN_WAIT2.
 *          FIN_WAIT2     FIN: a send (state still FIN_WAIT2), RNS_CTL_RESP_TIMER, state TIME_WAIT,
 *                        RNS_CTL_TIMEWAIT.
 *          CLOSING       ACK: state TIME_WAIT, RNS_CTL_TIMEWAIT.
 *          CLOSED, CLOSE_WAIT, TIME_WAIT: nothing.
 *        Every state change sets RNS_CTL_STATE on the record (set_state ran: the host zeroes
 *        request_retry_count) and RNS_EV_STATE on the flow.
 *   d_res is rns_tcp_flow_res: n_acks counts the segments sent.  Timers stay the host's, derived from
 *   the act bits and ack_timer.
 *   The reference's oddities are pinned, not corrected: a bare FIN to an Established socket gets no ACK
 *   at all; a FIN with payload there is ACKed without the FIN's + 1; the peer's ACK of our FIN fails
 *   seq_le(ack, snd_nxt) (snd_nxt is not advanced over the FIN), so it neither trims nor updates the
 *   window.  SYN_SENT (tcp_open is a blocking application call, and a peer's SYN|ACK carries options)
 *   and LISTEN (a listen socket is never a flow) are named but the host's.
 *   Unpinned: trim_head's assert (buf.rs:297), which the reference trips when acked exceeds the
 *   retransmit queue — reachable through the SynReceived record's snd_una, which holds the peer's
 *   sequence number; the device just counts acked.  And what the flow update leaves unpinned.
 * d_work / work_bytes: what rns_rx_tcp_conn_update_work gives for (n_pkts, n_flows). */
#define RNS_TCP_CLOSED     0u
#define RNS_TCP_CLOSE_WAIT 3u
#define RNS_TCP_LAST_ACK   4u
#define RNS_TCP_FIN_WAIT1  5u
#define RNS_TCP_FIN_WAIT2  6u
#define RNS_TCP_CLOSING    7u
#define RNS_TCP_TIME_WAIT  8u
#define RNS_TCP_SYN_SENT   9u
#define RNS_TCP_LISTEN     10u
typedef struct rns_tcp_ctl {   /* 16 bytes, host byte order */
    uint32_t flow;             /* whose template the segment is built from */
    uint32_t seq, ack_num;     /* as send_packet gives them at the moment of the send */
    uint16_t window;
    uint8_t  flags;            /* the TCP flags byte of the segment to send */
    uint8_t  act;              /* RNS_CTL_* */
} rns_tcp_ctl;
#define RNS_CTL_CONSUMED   1u   /* the segment was processed (== RNS_SEG_CONSUMED) */
#define RNS_CTL_SEND       2u   /* a segment is to be sent (== RNS_SEG_ACK) */
#define RNS_CTL_ACK_TIMER  4u   /* the delayed-ACK timer was started (== RNS_SEG_TIMER) */
#define RNS_CTL_RESP_TIMER 8u   /* set_response_timer was called */
#define RNS_CTL_TIMEWAIT   16u  /* the TIME_WAIT timer was set */
#define RNS_CTL_RESET      32u  /* an RST closed the socket */
#define RNS_CTL_STATE      64u  /* set_state ran */
#define RNS_EV_STATE       2u   /* rns_tcp_flow_res.events: the state changed */
#define RNS_STOP_TWICE     7u
int rns_rx_tcp_conn_update_dev(const rns_rx_tcp_meta *d_meta, uint32_t n_pkts, uint32_t n_flows,
                               const rns_tcp_flow *d_flow_in, const uint32_t *d_pend_in, uint32_t pend_cap,
                               rns_tcp_flow *d_flow_out, uint32_t *d_pend_out,
                               rns_tcp_ctl *d_ctl,          /* n_pkts */
                               rns_tcp_flow_res *d_res,     /* n_flows */
                               void *d_work, uint64_t work_bytes, void *stream);

/* The workspace of rns_rx_tcp_conn_update_dev (CPU only): the flow update's value and rules. */
int rns_rx_tcp_conn_update_work(uint32_t n_pkts, uint32_t n_flows, uint64_t *bytes);

/* Control-segment build: rns_tx_ack_build_dev's contract restated over rns_tcp_ctl records, whatever
 * wrote them (the connection update, the close step, a host that writes records for
 * response_timeout).  Control segment k is the k-th record i in ascending i with act & RNS_CTL_SEND and
 * f = flow < n_flows.  Its head, hl = d_head_len8[f] bytes at d_out + 64 * k, is the flow's template
 * verbatim except TCP [4..8] = seq, [8..12] = ack_num, [12] = 0x50, [13] = flags, [14..16] = window,
 * [16..18] = the checksum; IPv4: [2..4] = 40, [4..6] = ip_id_base + *d_ip_id_add (0 without it) + the
 * IPv4 segments among 0..k-1, mod 2^16, [10..12] = the header checksum; IPv6: [4..6] = 20.  For the
 * same ACKs the bytes are rns_tx_ack_build_dev's.  d_src[k] = i, d_len8[k] = hl, d_count = (segments,
 * IPv4 ones), always written.  The caps (out_cap), the counting-only mode (out_cap == 0 allows NULL
 * d_out / d_src / d_len8) and the malformed-template rule are the ACK build's; a record whose flags
 * carry SYN (0x02) is treated like a malformed template — slot and id kept, d_len8[k] = 0, nothing
 * written: a SYN needs the MSS option, which this form does not carry.
 * A NULL d_count; with n_ctl > 0 a NULL d_ctl / d_work, work_bytes below rns_tx_tcp_ctl_build_work's
 * or, with n_flows > 0, a NULL d_tmpl / d_head_len8 or tmpl_stride == 0; with out_cap > 0 a NULL d_out
 * / d_src / d_len8; a d_ctl / d_ip_id_add / d_out / d_src / d_count that is not 4-byte aligned or a
 * d_work that is not 8-byte aligned; or n_ctl > RNS_CHAIN_MAX_PACKETS is RNS_E_INVALID, all before the
 * device is touched. */
int rns_tx_tcp_ctl_build_dev(const rns_tcp_ctl *d_ctl, uint32_t n_ctl, uint32_t n_flows,
                             const uint8_t *d_tmpl, uint32_t tmpl_stride, const uint8_t *d_head_len8,
                             uint16_t ip_id_base, const uint32_t *d_ip_id_add /* optional device dword */,
                             void *d_work, uint64_t work_bytes,
                             uint8_t *d_out, uint32_t out_cap, uint32_t *d_src, uint8_t *d_len8,
                             uint32_t *d_count /* 2 */, void *stream);

/* The build's workspace in bytes for n_ctl records (CPU only): non-zero and monotone in n_ctl.
 * RNS_E_INVALID for a NULL bytes or n_ctl > RNS_CHAIN_MAX_PACKETS. */
int rns_tx_tcp_ctl_build_work(uint32_t n_ctl, uint64_t *bytes);

/* tcp_close (tcp.rs:195-224) for a batch of sockets, a lane per flow, no workspace.  d_op[f]: 0 none, 1
 * close.  For op 1 the state decides: ESTABLISHED sends and becomes FIN_WAIT1, CLOSE_WAIT sends and
 * becomes LAST_ACK, every other state (LISTEN too: its PORT_MAP removal is the host's) neither sends nor
 * changes.  A flow that sends gets d_ctl[f] = send_packet(FIN | ACK) computed BEFORE the state change,
 * as tcp.rs:211-219 orders it — flow = f, seq = snd_nxt, ack_num = rcv_nxt (+ 1 in CLOSE_WAIT when
 * rcv_max == rcv_nxt, never in ESTABLISHED), the window as in the flow update, flags = 0x11, act =
 * RNS_CTL_SEND | RNS_CTL_RESP_TIMER | RNS_CTL_STATE — and snd_nxt is not advanced (the reference does
 * not).  Every other flow (op 0, op 1 in a state that does not send, any other op) is copied and its
 * record is all zero.  d_flow_in == d_flow_out is allowed (any other overlap is not).  n_flows == 0 is
 * RNS_OK.  With n_flows > 0 a NULL d_flow_in / d_flow_out / d_op / d_ctl, a d_flow_in / d_flow_out /
 * d_ctl that is not 4-byte aligned, or n_flows >= 2^31 is RNS_E_INVALID, before the device is touched. */
int rns_tx_tcp_close_dev(const rns_tcp_flow *d_flow_in, rns_tcp_flow *d_flow_out, uint32_t n_flows,
                         const uint8_t *d_op, rns_tcp_ctl *d_ctl /* n_flows */, void *stream);

/* TCP send planning: tcp_write's window gate (tcp.rs:256-292) and retransmit (tcp.rs:329-348) on the
 * device, with the head fields send_packet sets (tcp.rs:402-447).  It reads the flow records where
 * rns_rx_tcp_flow_update_dev left them and writes exactly the descriptor set rns_tx_segment_dev takes,
 * so place -> update -> ACK build -> plan -> segment is one stream of launches.
 *   The send buffer: flow f's bytes lie contiguous in the arena rns_tx_segment_dev will get; the byte
 *     with sequence number d_sq_seq[f] is at d_sq_off[f] and d_sq_len[f] bytes follow it — the
 *     retransmit queue [snd_una, snd_nxt), then the data tcp_write has not sent.  The byte of sequence
 *     s is at sq_off + (s - sq_seq mod 2^32).  ACKs move snd_una only, so the host leaves the three
 *     arrays alone between batches.  inflight = snd_nxt - snd_una, a = snd_una - sq_seq, unsent =
 *     sq_len - a - inflight.  The planner never touches the arena.
 *   Stops, tested in this order; a stopped flow plans nothing, both its entries are empty and
 *   d_flow_out[f] == d_flow_in[f] bytewise:
 *     RNS_PLAN_STATE  state != RNS_TCP_ESTABLISHED.
 *     RNS_PLAN_BAD    mss == 0; sq_len, snd_wnd or inflight above 0x3fffffff; a > sq_len; a + inflight >
 *                     sq_len.  Inside this domain no seq_gt of the reference's loop wraps, so the
 *                     closed form below equals it; outside, the host decides.
 *     RNS_PLAN_TMPL   the template rule of rns_tx_ack_build_dev: hl = d_head_len8[f] is 40 or 60, hl <=
 *                     tmpl_stride, IPv4 (40) has t[0] == 0x45 and t[9] == 6, IPv6 (60) t[0] >> 4 == 6
 *                     and t[6] == 6, the TCP data offset is 5.
 *   Entries: flow f owns entries 2f and 2f + 1 of the E = 2 * n_flows entries, in that order — one of
 *   the orders the socket mutex allows between the timer thread and the writer, fixed here.
 *     2f, retransmit: if d_rexmit is non-NULL, d_rexmit[f] != 0 and inflight > 0, one segment of
 *       min(mss, inflight) bytes from the byte of snd_una.  Its sequence field is snd_nxt, NOT
 *       snd_una: the reference's send_packet puts send_next_seq into retransmitted data too
 *       (tcp.rs:439).  That is pinned as it is.
 *     2f + 1, new data (data = the unsent bytes): pieces of min(remaining, mss) go while
 *       !seq_gt(snd_nxt + piece, snd_una + snd_wnd); the first piece that fails ends the loop with why
 *       = RNS_PLAN_WINDOW (tcp_write would wait there).  So the entry is pay_off = the byte of snd_nxt,
 *       pay_len = the planned bytes — whole pieces, and the tail piece when everything fits — and mss.
 *       d_flow_out[f].snd_nxt += pay_len; every other field is copied.
 *   Template rows: the row of an entry with segments (d_tmpl_out + e * tmpl_stride) is the flow's
 *   template (d_tmpl + f * tmpl_stride) with TCP [4..8] = snd_nxt as it is before this flow's new
 *   data, [8..12] = rcv_nxt, [12] = 0x50, [13] = 0x18 (ACK|PSH), [14..16] = (0xffff - (rq_len &
 *   0xffff)) & 0xffff, and IPv4 [4..6] = ip_id_base + *d_ip_id_add + (the IPv4 segments of all earlier
 *   kept entries) mod 2^16; rns_tx_segment_dev adds j per segment, so the ids are NEXT_PACKET_ID's in
 *   entry order.  Only bytes [0, hl) of such a row are written; rows of empty entries are not written.
 *   Layout: d_seg_first is the exclusive prefix sum of the entries' segment counts (E + 1 entries),
 *   d_head_off[e] = head_first_off + the head bytes (segments * hl) of the earlier entries, held in 64
 *   bits.  Cap: an entry whose inclusive segment prefix exceeds seg_cap is dropped, and so is every
 *   later non-empty one — the kept entries are a prefix.  A dropped entry gets pay_len = 0; a flow
 *   whose new-data entry was dropped gets why = RNS_PLAN_CAP and snd_nxt not advanced; a dropped
 *   retransmit gives rexmit_bytes = 0.  (The prefix that decides this counts every entry at most seg_cap
 *   + 1 segments, mod 2^32: it is exact while those counts sum below 2^32.)  For the kept total N =
 *   d_n[0] (d_n[1]: the IPv4 segments among them), d_seg_first, d_head_off and the first (N + 63) / 64
 *   entries of d_blk_flow equal what rns_tx_segment_layout gives for the written pay_len / mss /
 *   head_len8, and d_blk_flow[b] = E for every block from there to (seg_cap + 63) / 64.  So
 *   rns_tx_segment_dev(n_flows = E) may be launched with n_seg = N after reading d_n, or with n_seg =
 *   seg_cap without reading anything: a segment at or past N finds no entry that covers it and gets
 *   RNS_TX_MALFORMED, no byte written (the one 64-segment block that straddles N walks d_seg_first to
 *   its end to learn that).
 *   Every output array is written in full on every call; d_head_len8_out[e] and d_mss_out[e] are the
 *   flow's values for both entries, d_pay_off is 0 for an empty entry.  n_flows == 0 writes
 *   d_seg_first[0] = 0, d_n = {0, 0} and d_blk_flow (zeros), and needs no other array.  Whatever the
 *   inputs hold, nothing outside the argument arrays is read or written.  The in and out arrays must
 *   not overlap.  The call allocates nothing: d_work is the caller's, at least rns_tx_tcp_plan_work
 *   bytes; its contents before and after the call mean nothing.
 * n_flows > 2^30, seg_cap > RNS_CHAIN_MAX_PACKETS, tmpl_stride == 0, a NULL d_seg_first or d_n, a NULL
 * d_blk_flow with seg_cap > 0, with n_flows > 0 any other NULL pointer but d_rexmit and d_ip_id_add, an
 * array that is not aligned to its elements (2 bytes for the u16 arrays, 4 for the u32 arrays, the flow
 * records and the results, 8 for the u64 arrays and d_work) or work_bytes below the need is
 * RNS_E_INVALID, all before the device is touched. */
typedef struct rns_tx_plan_res {   /* 16 bytes */
    uint32_t new_bytes;     /* bytes of new data planned (snd_nxt advanced by this) */
    uint32_t new_segs;      /* their segments */
    uint32_t rexmit_bytes;  /* bytes of the one retransmitted piece, 0 if none */
    uint8_t  why;           /* RNS_PLAN_* */
    uint8_t  pad[3];        /* zero */
} rns_tx_plan_res;
#define RNS_PLAN_NONE   0u  /* all queued data was planned (or there was none) */
#define RNS_PLAN_WINDOW 1u  /* tcp_write would wait: unsent bytes remain behind the window */
#define RNS_PLAN_STATE  2u
#define RNS_PLAN_BAD    3u
#define RNS_PLAN_TMPL   4u
#define RNS_PLAN_CAP    5u  /* seg_cap reached: the entry and every later one are dropped */
int rns_tx_tcp_plan_dev(const rns_tcp_flow *d_flow_in, rns_tcp_flow *d_flow_out, uint32_t n_flows,
                        const uint64_t *d_sq_off, const uint32_t *d_sq_seq, const uint32_t *d_sq_len, /* n_flows: send buffer */
                        const uint16_t *d_mss, const uint8_t *d_rexmit /* optional */,
                        const uint8_t *d_tmpl, uint32_t tmpl_stride, const uint8_t *d_head_len8,
                        uint16_t ip_id_base, const uint32_t *d_ip_id_add /* optional: one device dword added to the base */,
                        uint64_t head_first_off, uint32_t seg_cap,
                        /* outputs: rns_tx_segment_dev's descriptors over E = 2 * n_flows entries */
                        uint8_t *d_tmpl_out, uint8_t *d_head_len8_out, uint64_t *d_pay_off, uint32_t *d_pay_len,
                        uint16_t *d_mss_out, uint64_t *d_head_off, uint32_t *d_seg_first /* E + 1 */,
                        uint32_t *d_blk_flow /* (seg_cap + 63) / 64 */, uint32_t *d_n /* 2: segments, IPv4 segments */,
                        rns_tx_plan_res *d_res, void *d_work, uint64_t work_bytes, void *stream);

/* The workspace of rns_tx_tcp_plan_dev (CPU only): *bytes for n_flows flows, monotone.  A NULL bytes or
 * n_flows > 2^30 is RNS_E_INVALID. */
int rns_tx_tcp_plan_work(uint32_t n_flows, uint64_t *bytes);

/* Transmit finalize (SURVEY a6, §8f row 2 for whole datagrams): for each finished
 * outgoing IP datagram d_arena[d_off[i] .. + d_len[i]), the checksums the stack's
 * transmit path stores — tcp_output (tcp.rs:957-973: pseudo-header from the header's
 * source and destination, length as u16, field [16..18] of the segment), udp_output
 * (udp.rs:151-171, [6..8], 0 stored as is), icmp_output_v4 (icmp.rs:87-95, [2..4], no
 * pseudo-header), icmp_output_v6 (icmp.rs:97-112, [2..4], full length, protocol 58) and
 * ip_output_v4 (ip.rs:140-160, header[10..12] over IHL*4 bytes) — computed as if the
 * fields were zero (alloc_header zero-fills them, buf.rs:286-288) and stored big-endian
 * in place, with every pseudo-header formed on the device.  One pass over each
 * datagram's bytes.  Datagrams must not overlap.  d_status (optional) gets RNS_TX_*. */
#define RNS_TX_IP_FILLED      0x01u  /* IPv4 header checksum stored */
#define RNS_TX_L4_FILLED      0x02u  /* TCP / UDP / ICMP checksum stored */
#define RNS_TX_MALFORMED      0x80u  /* bad version / IHL / too short, or outside the arena: untouched */
int rns_tx_fill_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_off, const uint32_t *d_len,
                    uint32_t n, uint8_t *d_status, void *stream);

/* Transmit finalize of a PACKED transmit arena (the descriptor form of
 * rns_csum_batch_packed_dev: u16 lengths, d_blk_off[b] = offset of datagram 64*b, datagrams
 * back to back at 2^align_log2 boundaries, align_log2 >= 4): per datagram exactly what
 * rns_tx_fill_dev stores and reports (tcp.rs:957-973, udp.rs:151-171, icmp.rs:87-112,
 * ip.rs:140-160; both fields computed as zero, pseudo-headers from the header's own
 * addresses).  One wave streams each 64-datagram block as whole 1 KiB rows (the rows kernel)
 * while each owner holds its datagram's header chunks and stores its two fields with one
 * 2-byte store each.  len_hint = the typical datagram length (row depth; 0 = unknown).
 * d_status optional.  align_log2 < 4 is RNS_E_INVALID. */
int rns_tx_fill_packed_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_blk_off, const uint16_t *d_len16,
                           uint32_t align_log2, uint32_t n, uint8_t *d_status, uint32_t len_hint, void *stream);

/* Transmit finalize of datagrams held as NetBuffer chains — the reference's own transmit layout
 * (buf.rs:262-291, 385-420): datagram i = the CSR chain of rns_csum_chain_dev (fragments
 * [d_first[i], d_first[i+1]) of (d_frag_off, d_frag_len)), whose FIRST fragment is the head
 * fragment alloc_header built — the IP header and, behind it, the L4 header (both prepended
 * into one fragment) — followed by the payload fragments.  Per datagram what tcp_output /
 * udp_output / icmp_output_* and ip_output_v4 store (tcp.rs:957-973, udp.rs:151-171,
 * icmp.rs:87-112, ip.rs:140-160): the L4 checksum = compute_buffer_ones_comp(pseudo-header,
 * [head[hdr..], payload...]) folded per fragment as the reference folds it (an odd-length
 * fragment pads its last byte), pseudo-header from the head's addresses and the chain's total
 * length; the IPv4 header checksum over head[..IHL*4]; both fields computed as zero and stored
 * big-endian into the head fragment.  Only head bytes are written.  d_status (optional) gets
 * RNS_TX_*: MALFORMED (untouched) for a malformed range, no fragments, a fragment outside the
 * arena, or a head that does not hold the IP header; no L4 fill for a protocol the stack does
 * not checksum, a segment too short for its field, or a field past the head fragment.  Heads
 * of consecutive datagrams back to back in a header region and payloads back to back at
 * 16-byte-aligned starts (the shape of RNS_FLAG_CHAIN_TX_PACKED; heads of at most 80 bytes from
 * their 16-byte boundary, at most 4 payload fragments forming a run) stream as rows; any other
 * 64-datagram block takes an exact per-datagram loop (same results, slower).  n_pkts >
 * RNS_CHAIN_MAX_PACKETS is RNS_E_INVALID. */
int rns_tx_fill_chain_dev(uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_frag_off, const uint32_t *d_frag_len,
                          uint32_t n_frags, const uint32_t *d_first, uint32_t n_pkts, uint8_t *d_status, void *stream);

/* The same finalize over COMPACT descriptors, for the layout a batching transmit path builds
 * itself: datagram i = [head] or [head, payload], the heads of a 64-datagram block back to back
 * in a header region and its payloads back to back at 2^pay_align_log2 boundaries in a payload
 * region, so every offset is implied by the lengths.  Within block b: head 64b starts at
 * d_head_blk_off[b] and head i where head i-1 ends (no padding); payload 64b starts at
 * d_pay_blk_off[b] and payload i at the end of payload i-1 rounded up to 2^pay_align_log2 (each
 * payload occupies its length padded to that alignment; a zero-length payload occupies nothing
 * and means a head-only datagram).  The blocks' offsets are independent of each other, as in
 * rns_csum_batch_packed_dev.  Descriptors: 3 B per datagram (u8 head length, u16 payload length)
 * + 16 B per 64 datagrams — about 3.25 B per datagram against the CSR form's 28 B per
 * [head, payload] datagram.  With ho_i / po_i the implied offsets, the bytes stored and
 * d_status[i] (optional) are exactly those of rns_tx_fill_chain_dev for the chain
 * [(ho_i, head_len_i)] plus [(po_i, pay_len_i)] when pay_len_i > 0: the same RNS_TX_* bits and
 * rejections (a head that does not hold its IP header, a head of length 0, anything outside the
 * arena: RNS_TX_MALFORMED, untouched; an L4 field past the head: no L4 fill).  Only head bytes
 * are written; heads and payloads of different datagrams must not overlap.  A block with a head
 * past 80 bytes from its 16-byte boundary, or whose payload block offset is not 16-byte aligned
 * (in memory: arena base + offset), takes the exact per-datagram loop (same results, slower).
 * pay_align_log2 outside 4..12 or n > RNS_CHAIN_MAX_PACKETS is RNS_E_INVALID. */
int rns_tx_fill_chain_packed_dev(uint8_t *d_arena, uint64_t arena_bytes,
                                 const uint64_t *d_head_blk_off, /* offset of the head of datagram 64*b */
                                 const uint8_t *d_head_len8,     /* head fragment length per datagram, 0..255 */
                                 const uint64_t *d_pay_blk_off,  /* offset of the payload of datagram 64*b */
                                 const uint16_t *d_pay_len16,    /* payload length per datagram, 0 = head only */
                                 uint32_t pay_align_log2,        /* payloads start at 2^this boundaries, 4..12 */
                                 uint32_t n, uint8_t *d_status, void *stream);

/* The same finalize for datagrams held in POOL BUFFERS as the reference's transmit path leaves them
 * — append_from_slice (buf.rs:385-420) fills whole buffers from offset 0 and a last one with the
 * remainder, alloc_header (buf.rs:262-291) prepends a buffer whose data sits at its end — over the
 * compact descriptors of rns_rx_verify_pool_dev.  d_pool (16-byte aligned) holds buffers of
 * 2^buf_log2 bytes (8 <= buf_log2 <= 15, so every u8 head length fits a buffer; the reference's
 * FRAGMENT_SIZE is 2^9), buffer k = d_pool[k << buf_log2 .. ).  Datagram i names
 * nf_i = 1 + ceil(pay_len_i / 2^buf_log2) buffers, d_buf_idx[first_i .. first_i + nf_i), with first_i
 * = d_blk_first[i / 64] + the sum of nf_k over the datagrams k of i's 64-datagram block before i
 * (the blocks' entries are independent of each other).  The first is the head buffer: the head
 * fragment is its LAST head_len_i bytes, offset (idx << buf_log2) + 2^buf_log2 - head_len_i.  The
 * others are payload buffers read from their start, all full but the last, which holds the
 * remainder.  Descriptors: 3 B per datagram + 4 B per buffer + 4 B per 64 datagrams — 19 B for a
 * 1500-byte datagram in 512-byte buffers against the CSR form's 52 B.
 * The form is defined by the CSR chain it expands to: the bytes stored and d_status[i] (optional)
 * are exactly what rns_tx_fill_chain_dev gives for that chain on the same memory — the head's L4
 * part folded as a fragment of its own (an odd length zero-padded), head_len 0 or a head that does
 * not hold its IP header RNS_TX_MALFORMED, no L4 fill for a field that runs past the head.  A
 * datagram with a buffer whose used bytes end past pool_bytes, or with first_i + nf_i > n_frags, is
 * RNS_TX_MALFORMED and untouched, that datagram only.  Only head bytes are written (at most the
 * two 2-byte fields): a head buffer must not be named anywhere else in the batch; payload buffers
 * may be shared between datagrams.  Heads of any length and alignment take the same path: there
 * is no exact per-datagram loop.
 * n_pkts == 0 is RNS_OK; buf_log2 outside 8..15, a NULL d_pool / d_blk_first / d_head_len8 /
 * d_pay_len16, a NULL d_buf_idx with n_frags > 0, n_pkts > RNS_CHAIN_MAX_PACKETS or a d_pool that is
 * not 16-byte aligned is RNS_E_INVALID, all before the device is touched. */
int rns_tx_fill_pool_dev(uint8_t *d_pool, uint64_t pool_bytes, uint32_t buf_log2,
                         const uint32_t *d_buf_idx, uint32_t n_frags,
                         const uint32_t *d_blk_first,   /* (n_pkts + 63) / 64 entries */
                         const uint8_t  *d_head_len8,   /* head length per datagram, 0..255 */
                         const uint16_t *d_pay_len16,   /* payload length per datagram, 0 = head only */
                         uint32_t n_pkts, uint8_t *d_status /* optional */, void *stream);

/* Host helper for the pool transmit form (CPU only), rns_rx_pool_layout with the + 1 for the head
 * buffer: from the n payload lengths, blk_first ((n + 63) / 64 entries), optionally first[0..n]
 * (the CSR index of the expanded chains) and *n_frags.  RNS_E_INVALID if the fragment total does
 * not fit 32 bits or buf_log2 is outside 8..15. */
int rns_tx_pool_layout(const uint16_t *pay_len16, uint64_t n, uint32_t buf_log2,
                       uint32_t *blk_first, uint32_t *first /* optional, n + 1 */, uint64_t *n_frags);

/* TCP segmentation offload: tcp_write's segment loop (tcp.rs:256-285) on the device.  The reference
 * cuts one send into send_mss pieces and sends each through send_packet -> tcp_output -> ip_output
 * with the same ports, ack, window, flags and addresses; retransmit (tcp.rs:329-348) is the same with
 * one piece.  So a "flow" — one tcp_write call — is a template head (IP + TCP header, finished but
 * for the fields below), its data where it lies in the arena (any byte alignment), its mss and the
 * place its heads go: flow f has nseg_f = ceil(pay_len_f / mss_f) segments, segment j carries
 * data[j * mss .. min((j + 1) * mss, pay_len)) and its head, hl = d_head_len8[f] bytes, is written at
 * d_head_off[f] + j * hl.  The head is the template (d_tmpl + f * tmpl_stride) copied verbatim except
 *   IPv4 (ip.rs:140-160): [2..4] = hl + seglen, [4..6] = the template's id + j (mod 2^16),
 *                         [10..12] = the header checksum;
 *   IPv6 (ip.rs:164-177): [4..6] = the TCP header length + seglen;
 *   TCP at the IP header's end (tcp.rs:938-976): [4..8] = the template's seq + j * mss (mod 2^32),
 *                         [16..18] = the checksum (pseudo-header from the template's addresses, the
 *                         length TCP header + seglen as u16, protocol 6).
 * Flags, ack, window, options, TTL and everything else are the template's in EVERY segment: the
 * reference sends ACK|PSH on each piece, so no flag is cleared on the segments before the last as a
 * NIC's TSO would.  Whatever the template's two checksum fields hold is ignored.
 * The form is defined by what it expands to: after the call the head range and
 * d_status[d_seg_first[f] + j] (optional) hold the head built as above with both checksum fields
 * zero, and then exactly what rns_tx_fill_chain_dev stores and reports for the chain
 * [(head_off_f + j * hl, hl), (pay_off_f + j * mss, seglen)].  The TCP header has even length, so
 * every fragment the reference would fold over the same bytes but the last has even length too
 * (the head's L4 part, then 512-byte payload fragments), and folding per fragment then equals
 * folding the whole: the value is compute_buffer_ones_comp over the reference's own fragments.
 * d_seg_first is the CSR index of segments over flows (n_flows + 1 entries), d_blk_flow[b] the flow
 * that holds segment 64 * b ((n_seg + 63) / 64 entries): rns_tx_segment_layout computes both.
 * A flow is rejected — every one of its segments RNS_TX_MALFORMED, no byte of its head range
 * written, that flow only — unless hl <= tmpl_stride; the template is IPv4 with t[0] == 0x45 and
 * t[9] == 6 (IP header 20 bytes) or IPv6 with t[0] >> 4 == 6 and t[6] == 6 (40 bytes); the TCP data
 * offset at t[iphdr + 12] >> 4 is >= 5 and iphdr + 4 * doff == hl; mss >= 1 and hl + mss <= 65535;
 * d_seg_first[f + 1] - d_seg_first[f] == nseg_f and d_seg_first[f + 1] <= n_seg; the data range and
 * the head range lie inside the arena.  A segment that no well-formed flow covers is
 * RNS_TX_MALFORMED.  Whatever the descriptors hold, nothing outside the arena and the descriptor
 * arrays is read or written.  Only head ranges are written: they must not overlap each other, any
 * data or the templates.  Descriptors: 27 B + the template per flow and 4 B per 64 segments, nothing
 * per datagram.
 * n_flows == 0 or n_seg == 0 is RNS_OK; a NULL d_arena / d_tmpl / d_head_len8 / d_pay_off /
 * d_pay_len / d_mss / d_head_off / d_seg_first / d_blk_flow, tmpl_stride == 0 or n_seg >
 * RNS_CHAIN_MAX_PACKETS is RNS_E_INVALID, all before the device is touched. */
int rns_tx_segment_dev(uint8_t *d_arena, uint64_t arena_bytes,
                       const uint8_t  *d_tmpl, uint32_t tmpl_stride, /* template f at d_tmpl + f * tmpl_stride */
                       const uint8_t  *d_head_len8,  /* n_flows: template / head length */
                       const uint64_t *d_pay_off,    /* n_flows: the send's data in the arena */
                       const uint32_t *d_pay_len,    /* n_flows: data bytes; 0 = no segments */
                       const uint16_t *d_mss,        /* n_flows */
                       const uint64_t *d_head_off,   /* n_flows: where the flow's heads go, back to back */
                       const uint32_t *d_seg_first,  /* n_flows + 1: CSR of segments over flows */
                       const uint32_t *d_blk_flow,   /* (n_seg + 63) / 64: the flow that holds segment 64 * b */
                       uint32_t n_flows, uint32_t n_seg, uint8_t *d_status /* optional, n_seg */, void *stream);

/* Host helper for the segmentation form (CPU only): from the n_flows data lengths, mss and head
 * lengths and the first head's offset, seg_first (n_flows + 1), head_off (n_flows: the flows' heads
 * back to back in flow order), *n_seg, *head_end (just past the last head) and, when blk_flow is
 * non-NULL, its (n_seg + 63) / 64 entries — call it once with blk_flow NULL for *n_seg, then again
 * with the array.  mss == 0 with pay_len > 0, or a segment total past RNS_CHAIN_MAX_PACKETS, is
 * RNS_E_INVALID. */
int rns_tx_segment_layout(const uint32_t *pay_len, const uint16_t *mss, const uint8_t *head_len8, uint32_t n_flows,
                          uint64_t head_first_off, uint32_t *seg_first, uint64_t *head_off,
                          uint32_t *blk_flow /* optional */, uint64_t *n_seg, uint64_t *head_end);

/* The CSR chains the segmentation form expands to (CPU only; two fragments per segment: its head,
 * its data slice), for rns_io_send_batch_chain and rns_tx_fill_chain_dev: frag_off / frag_len get
 * 2 * n_seg entries, first n_seg + 1.  RNS_E_INVALID if the flows do not have n_seg segments in all
 * or an mss is 0 with data to send. */
int rns_tx_segment_chains(const uint64_t *pay_off, const uint32_t *pay_len, const uint16_t *mss,
                          const uint8_t *head_len8, const uint64_t *head_off, uint32_t n_flows, uint64_t n_seg,
                          uint64_t *frag_off, uint32_t *frag_len, uint32_t *first);

/* Host helper for the compact chain form (CPU only): given the n head and payload lengths, the
 * payload alignment (4..12) and the first head's and first payload's offsets, writes the
 * (n + 63) / 64 block offsets of each region, the offsets just past the last head and the last
 * payload's padded end (*head_end, *pay_end), and optionally (non-NULL) every datagram's head
 * and payload offset. */
int rns_tx_chain_packed_layout(const uint8_t *head_len8, const uint16_t *pay_len16, uint64_t n,
                               uint32_t pay_align_log2, uint64_t head_first_off, uint64_t pay_first_off,
                               uint64_t *head_blk_off, uint64_t *pay_blk_off, uint64_t *head_off /*opt*/,
                               uint64_t *pay_off /*opt*/, uint64_t *head_end, uint64_t *pay_end);

/* Tuning entry (bench / tests): explicit kernel shape.  variant bit 0: 0 = group
 * kernel (one lane stores each result), 1 = rounds kernel (a wave owns 64
 * consecutive packets, one coalesced result store); bit 1: nontemporal packet
 * loads; bit 2: mixed kernel (rounds kernel that sorts each wave's 64 packets
 * into size classes, each with its own shape; G and U are ignored); bit 3 (with
 * bit 0 only): rounds kernel with every round of a batch in flight (G <= 8, U <= 2);
 * bit 4 (with bit 0 only, not with bit 3): rounds kernel that loads the next wave
 * batch's descriptors before the current batch's data (G <= 8, U <= 2);
 * bits 8-11: at most that many 4-wave workgroups per CU (an occupancy cap, by LDS
 * reservation; 0 = none).
 * lanes_per_packet in {4,8,16,32,64} (2 too for the rounds kernel); unroll (16-byte
 * chunks in flight per lane per pass) in {1,2,4,8}; max_blocks = grid cap (0 = no
 * grid-stride loop). */
int rns_csum_batch_dev_cfg(const uint8_t *d_arena, uint64_t arena_bytes, const uint64_t *d_off,
                           const uint32_t *d_len, const uint16_t *d_seed, uint16_t *d_out, uint32_t n,
                           uint32_t flags, uint32_t variant, uint32_t lanes_per_packet, uint32_t unroll,
                           uint32_t max_blocks, uint32_t *d_bad, void *stream);

/* Host-resident batch through a staging context: chunked H2D copies, kernels and
 * D2H copies of the 2-byte results overlapped on several streams of `device`.
 * Offsets must be ascending.  Synchronous (returns when h_out is filled).
 * The whole batch is validated before anything is queued: a packet with
 * (offset mod 256) + length > chunk_bytes returns RNS_E_TOOLARGE (and out-of-arena /
 * descending descriptors RNS_E_BOUNDS / RNS_E_ORDER) with h_out untouched.
 * For full PCIe rate allocate h_arena with rns_host_alloc (pinned).  A context
 * serialises its own calls (internal mutex); use one per thread for concurrency. */
typedef struct rns_host_ctx rns_host_ctx;
int rns_host_ctx_create(int device, uint64_t chunk_bytes, uint32_t nstreams, rns_host_ctx **out);
int rns_host_ctx_destroy(rns_host_ctx *ctx);
int rns_csum_batch_host(rns_host_ctx *ctx, const uint8_t *h_arena, uint64_t arena_bytes,
                        const uint64_t *h_off, const uint32_t *h_len, const uint16_t *h_seed,
                        uint16_t *h_out, uint32_t n, uint32_t flags);

/* Multi-GPU batches.  Packets are independent, so the
 * batch is cut into contiguous packet ranges of about equal bytes, one per GPU,
 * with no collective: each GPU's results go straight to their slice of the output.
 * rns_csum_batch_multi_host: a host-resident batch over one staging context per
 * device (devices[] may repeat a device), ranges run concurrently, synchronous.
 * rns_csum_batch_multi_dev: each GPU's shard is already in its own HBM; launches
 * every shard on its device and stream and returns (asynchronous, like
 * rns_csum_batch_dev); the calling thread's current device is restored. */
typedef struct rns_multi_ctx rns_multi_ctx;
int rns_multi_ctx_create(const int *devices, uint32_t ndev, uint64_t chunk_bytes, uint32_t nstreams,
                         rns_multi_ctx **out);
int rns_multi_ctx_destroy(rns_multi_ctx *ctx);
int rns_csum_batch_multi_host(rns_multi_ctx *ctx, const uint8_t *h_arena, uint64_t arena_bytes,
                              const uint64_t *h_off, const uint32_t *h_len, const uint16_t *h_seed,
                              uint16_t *h_out, uint32_t n, uint32_t flags);
typedef struct rns_dev_batch {
    int device;                 /* HIP device of this shard */
    const uint8_t *d_arena;     /* this shard's arena, on `device` */
    uint64_t arena_bytes;
    const uint64_t *d_off;
    const uint32_t *d_len;
    const uint16_t *d_seed;     /* NULL: seed 0 */
    uint16_t *d_out;
    uint32_t n;
    uint32_t len_hint;          /* as rns_csum_batch_dev */
    uint32_t *d_bad;            /* optional */
    void *stream;               /* a stream of `device` (NULL: its default stream) */
} rns_dev_batch;
int rns_csum_batch_multi_dev(const rns_dev_batch *batches, uint32_t nbatches, uint32_t flags);

/* Batched datagram I/O.  The reference reads / writes one
 * packet per call on the TUN fd (recv_packet netif.rs:65-83 -> tun_recv tun.c:84-86;
 * send_packet netif.rs:85-98 -> tun_send tun.c:88-90).  rns_io_recv_batch waits up
 * to timeout_ms for the first datagram, then reads every datagram already queued
 * (up to max_pkts) into consecutive slot_bytes slots of h_arena (2048 = the
 * reference's MRU, netif.rs:66); h_off/h_len describe them.  A datagram longer
 * than its slot is dropped (on socket fds recv(MSG_TRUNC) reports its full length),
 * never handed on truncated; max_pkts is capped at INT_MAX.  Returns the number of
 * datagrams (0 on timeout) or RNS_E_IO.  Works on a TUN fd or any datagram fd; on a
 * socket fd up to 64 datagrams per recvmmsg call.
 * rns_io_send_batch writes n datagrams (sendmmsg on a socket fd, one writev per datagram
 * on a TUN fd); returns how many were written. */
int rns_io_recv_batch(int fd, uint8_t *h_arena, uint64_t slot_bytes, uint32_t max_pkts, uint64_t *h_off,
                      uint32_t *h_len, int timeout_ms);
int rns_io_send_batch(int fd, const uint8_t *h_arena, const uint64_t *h_off, const uint32_t *h_len, uint32_t n);
/* Batched send_packet of NetBuffer chains (netif.rs:85-98: to_iovec over the fragments, then
 * tun_send's writev, tun.c:88-90): datagram i = fragments [h_first[i], h_first[i+1]) of
 * (h_frag_off, h_frag_len), at least one and at most RNS_IO_MAX_FRAGS of them (the reference's
 * MAX_VECS, netif.rs:22), sent as ONE datagram gathered from its fragments — sendmmsg with one message per
 * datagram on a socket fd, one writev per datagram on a TUN fd.  The chains of
 * rns_tx_fill_chain_dev go out as they are (heads in a header region, payloads elsewhere).
 * Returns the datagrams sent; a malformed range or too many fragments is RNS_E_INVALID before
 * anything is sent. */
#define RNS_IO_MAX_FRAGS 8u
int rns_io_send_batch_chain(int fd, const uint8_t *h_arena, const uint64_t *h_frag_off, const uint32_t *h_frag_len,
                            const uint32_t *h_first, uint32_t n_pkts);

/* rns_io_send_batch_chain fed from the compact form of rns_tx_fill_pool_dev (buffers of 2^buf_log2
 * bytes, 8..15): datagram i goes out as one message gathered from the last h_head_len8[i] bytes of
 * its head buffer and its payload buffers, all full but the last — sendmmsg on a socket fd, one
 * writev per datagram on a TUN fd.  A datagram with more than RNS_IO_MAX_FRAGS fragments (the head
 * included) or with a head length of 0 is RNS_E_INVALID before anything is sent.  Returns the
 * datagrams sent. */
int rns_io_send_batch_pool(int fd, const uint8_t *h_pool, uint32_t buf_log2, const uint32_t *h_buf_idx,
                           const uint32_t *h_blk_first, const uint8_t *h_head_len8,
                           const uint16_t *h_pay_len16, uint32_t n_pkts);

/* Batched receive straight into a PACKED arena (the descriptor form of
 * rns_rx_verify_packed_dev): every queued datagram (after waiting up to timeout_ms for the
 * first) goes to the next 16-byte boundary of h_arena, as long as a datagram of mru bytes
 * (<= 65535; the reference's MRU is 2048, netif.rs:66) still fits behind it and fewer than
 * max_pkts were read.  h_len16[i] = datagram i's length, h_blk_off[b] = the offset of
 * datagram 64*b, *h_end = the arena bytes used (the last datagram's end rounded up to 16:
 * what a copy to the GPU needs).  A datagram longer than mru is dropped.  On a socket fd
 * batches of up to 64 datagrams take one recvmmsg each; a TUN fd takes one read per
 * datagram.  Returns the number of datagrams (0 on timeout) or RNS_E_IO. */
int rns_io_recv_batch_packed(int fd, uint8_t *h_arena, uint64_t arena_bytes, uint32_t mru, uint32_t max_pkts,
                             uint16_t *h_len16, uint64_t *h_blk_off, uint64_t *h_end, int timeout_ms);

/* Batched recv_packet into NetBuffer chains (netif.rs:65-83: new_prealloc(MRU), readv over the
 * fragments, trim_tail), the receive twin of rns_io_send_batch_chain: h_pool is a pool of
 * buf_bytes-byte buffers (512 = the reference's FRAGMENT_SIZE), h_free[0..n_free) the indices of
 * the free ones.  After waiting up to timeout_ms for the first datagram, every queued datagram is
 * read into the next ceil(mru / buf_bytes) free buffers (at most RNS_IO_MAX_FRAGS, else
 * RNS_E_INVALID) — recvmmsg with one iovec list per message on a socket fd, up to 64 datagrams
 * per call; one readv per datagram on a TUN fd — and keeps the ceil(len / buf_bytes) buffers it
 * filled, the last fragment's length the remainder.  The call goes on while that many free
 * buffers remain and fewer than max_pkts datagrams were read.  On return h_free is permuted: its
 * first *n_frags_out entries are the buffers now in use, in fragment order (h_frag_off[j] =
 * h_free[j] * buf_bytes, h_frag_len[j]), the rest are still free; h_first (max_pkts + 1 entries)
 * is the CSR index of the datagrams: what rns_rx_verify_chain_dev takes once the pool is on the
 * device.  A datagram longer than mru is dropped and takes no buffer (MSG_TRUNC on sockets; a
 * TUN read is offered mru + 1 bytes); a zero-length datagram is skipped and those after it are
 * kept (a recvmmsg round of nothing but empty reads ends the call: a closed stream peer reads
 * that way for ever).  Returns the number of datagrams (0 on timeout) or RNS_E_IO. */
int rns_io_recv_batch_chain(int fd, uint8_t *h_pool, uint32_t buf_bytes, uint32_t *h_free, uint32_t n_free,
                            uint32_t mru, uint32_t max_pkts, uint64_t *h_frag_off, uint32_t *h_frag_len,
                            uint32_t *h_first /* max_pkts + 1 */, uint32_t *n_frags_out, int timeout_ms);

/* rns_io_recv_batch_chain with the compact outputs of rns_rx_verify_pool_dev, buffers of
 * 2^buf_log2 bytes (6..15): h_free is permuted exactly as there, and its first *n_frags_out entries
 * ARE d_buf_idx; h_len16[i] (max_pkts entries) = datagram i's length, h_blk_first[b]
 * ((max_pkts + 63) / 64 entries) = the first fragment of datagram 64*b.  The same receive loop: the
 * same drops, skips, caps and return values.  mru <= 65535, else RNS_E_INVALID. */
int rns_io_recv_batch_pool(int fd, uint8_t *h_pool, uint32_t buf_log2, uint32_t *h_free, uint32_t n_free,
                           uint32_t mru, uint32_t max_pkts, uint16_t *h_len16, uint32_t *h_blk_first,
                           uint32_t *n_frags_out, int timeout_ms);

/* Pinned host memory for arenas handed to rns_csum_batch_host. */
int rns_host_alloc(uint64_t bytes, void **out);
int rns_host_free(void *p);

/* Deterministic synthetic packet bytes on the device: splitmix64 stream,
 * little-endian words, word i = mix(seed + (i+1)*0x9E3779B97F4A7C15) — the
 * generator oracle/oracle.py splitmix64_bytes restates on the CPU. */
int rns_fill_splitmix64_dev(uint8_t *d_buf, uint64_t nbytes, uint64_t seed, void *stream);

/* ---- introspection ------------------------------------------------------- */
int rns_abi_version(void);
const char *rns_strerror(int status);
const char *rns_build_info(void);
/* Kernel and shape rns_csum_batch_dev picks for a typical packet length. */
const char *rns_csum_shape_name(uint32_t len_hint);
int rns_device_count(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RNS_CHECKSUM_H */
