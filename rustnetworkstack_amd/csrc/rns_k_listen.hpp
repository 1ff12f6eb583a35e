// TCP listen responder over pool buffers (rns_rx_tcp_listen_pool_dev): tcp_input's branch for a segment whose
// key is not in PORT_MAP (tcp.rs:579-615) and handle_new_connection (tcp.rs:894-936) — the RST|ACK for a
// stray segment, the SYN-ACK and the new socket's state for a SYN to a listening port — built on the device
// from the placement's meta records.  It takes over the branch the placement leaves to the host.
// (The kernels of k_listen.hip alone: they are no templates.  Their arguments are in rns_k_args.hpp.)
#pragma once

#include "rns_k_args.hpp"

namespace rns {

// ---------------------------------------------------------------------------
// The reference inserts the new socket into PORT_MAP at a key's first SYN, so every later segment of that
// key in the batch finds it and takes neither this branch nor a reply.  For a batch processed in index
// order that is one number per key: s(key), the smallest index among the candidates (SYNs to a listening
// port) with that key.  Grid-wide ordering comes from the launch boundaries on the one stream only:
//   1. listen_classify_kernel  a lane per datagram, a wave per 64-datagram block (the unit of d_blk_first),
//                              four blocks per workgroup: decides unmatched / candidate from the meta, the
//                              listen table and the first buffer, leaves a dword per datagram in the
//                              workspace, and a candidate inserts its key into the open-addressing table
//                              (cleared to all ones by a fill kernel before the launch).
//   2. listen_resolve_kernel   the same decomposition: an unmatched datagram looks s(key) up, decides
//                              SYN / HOST / LATER / RST, a first SYN walks its options; the workgroup's
//                              sums of (replies, IPv4 replies) and (accepts, 0).
//   3. scan2_parts_kernel      (rns_k_scan.hpp, through k_scan.hip) over each of the two sum arrays.
//   4. listen_build_kernel     scans its workgroup again, applies reply_cap, and the datagram's own lane
//                              composes its reply in registers (rns_k_tcp_head.hpp's helpers, both checksums
//                              filled), stores it as whole dwords, and stores the accept record.
//
// The table and its atomics.  A slot is (resident | tag << 32, first): the resident is the index of one datagram
// whose key the slot stands for and the tag that key's hash, claimed together by one 64-bit compare-and-swap on
// the empty value; first is lowered by an atomic min with every candidate of that key.  A slot's key is never
// stored: where the tag equals the asking key's hash it is derived again from the resident's meta record and
// first buffer, inputs that no kernel of the call writes, so a probe that meets a resident depends on nothing
// another lane has stored but the word the atomic returned.  (The tag is a filter only: a probe that walks over
// other keys' slots, the common case in a flood of distinct sources, derives nothing; without it every such
// step cost the resident's fragment count — up to 63 lengths — and two more lines, 1008 us for 2^20 SYNs.)
// Which datagram becomes a slot's resident, and which slot a key lands in, is whatever the atomics gave; the
// minimum index per key is not, and it is the only thing read back (by the next launch).  This is the flow
// update's rule: no atomic's order reaches an output, so the same inputs give the same bytes on every run.
// Slots >= 2 * n_pkts and at most one slot per candidate: a probe meets an empty slot within the table.
//
// Lane to reply: one lane per reply, the lane of its datagram.  Everything a reply is made of (meta, source
// address, ranks) is already in that lane's registers after the scan, a reply is 10 to 16 dwords, and the
// replies of a wave are consecutive ranks: its stores fall into one contiguous run of at most 4 KiB of d_out.
// The guides' ideal store has lane i at base + i * sizeof(T); here each store instruction has its lanes 64
// bytes apart instead, the uncoalesced pattern the guides leave to L2, and what keeps it cheap is that a
// 64-byte slot is written by one lane's 10 to 16 back-to-back stores and by nobody else.  A few lanes per
// slot would make each store instruction lane-consecutive, at the price of moving up to 16 dwords per reply
// through LDS and a second pass over the ranks, for 40 to 64 bytes per reply next to the 24 B of meta, the
// header line and the table words the same reply reads; d_out is 4-byte aligned only, so wider stores are
// not to be had either way.  The ACK build, the floor this entry is measured against, made the same choice
// for the same slots.
// ---------------------------------------------------------------------------
constexpr uint32_t kListenWaves = kScanBlock / 64;

// the workspace's dword per datagram: the RNS_CONN_* bits decided so far, then
constexpr uint32_t kListenRecCand = 0x100u, kListenRecV4 = 0x200u;  // a candidate; an IPv4 datagram
constexpr int kListenRecMssShift = 16;                              // a first SYN's max_segment_size

// What the responder needs of an unmatched datagram.
struct ListenSeg {
    uint32_t key[6];  // the flow table's six dwords
    uint32_t seq, ack, window, flags, ip_hdr, tcp_hdr;
    const uint32_t *h;  // its first buffer
    bool v6;
};

// The first fragment of datagram p in d_buf_idx for a lane that is not p's own (a slot's resident): its block's
// first plus the fragments of the datagrams before it in the block.
__device__ __forceinline__ uint64_t listen_gi(const PoolRx &rx, uint64_t p)
{
    const uint32_t bmask = (1u << rx.blog) - 1u;
    uint64_t gi = rx.blk_first[p >> 6];
    for (uint64_t j = p & ~63ull; j < p; ++j)
        gi += (rx.len16[j] + bmask) >> rx.blog;
    return gi;
}

// Datagram p (p < n, its first fragment at d_buf_idx[gi]) as an unmatched segment: false for everything else.
// The meta's claims are checked again before a header dword is read: the fragments inside d_buf_idx, the first
// buffer's bytes inside the pool, T >= 16 so that h[0..3] are the datagram's, the IP header length the one
// the first dword gives, 20 <= tcp_hdr <= 60 and ip_hdr + tcp_hdr <= T.  Then ip_hdr + tcp_hdr <= 120 lies
// inside the first buffer (B >= 128) and inside the datagram, and an IPv6 source address (T >= 60) too.
__device__ __forceinline__ bool listen_seg(const ListenArgs &a, uint64_t p, uint64_t gi, ListenSeg &s)
{
    const uint32_t *m = a.meta + p * 6;
    const uint32_t misc = m[5], place = misc >> 24;
    if ((place & (RNS_PLACE_TCP | RNS_PLACE_FLOW)) != RNS_PLACE_TCP)
        return false;
    const uint32_t B = 1u << a.rx.blog, T = a.rx.len16[p], nf = (T + B - 1u) >> a.rx.blog;
    if (nf == 0 || gi + nf > a.rx.n_frags || T < 16u)
        return false;
    const uint64_t s0 = static_cast<uint64_t>(a.rx.buf_idx[gi]) << a.rx.blog;
    const uint32_t len0 = min(T, B);
    if (s0 > a.rx.pool_bytes || len0 > a.rx.pool_bytes - s0)
        return false;
    s.h = reinterpret_cast<const uint32_t *>(a.rx.pool + s0);
    const uint32_t ver = (s.h[0] >> 4) & 0xfu;
    const IpHead ip = ip_head(s.h);
    s.ip_hdr = (misc >> 8) & 0xffu;
    s.tcp_hdr = (misc >> 16) & 0xffu;
    if ((ver != 4u && ver != 6u) || ip.ip_hdr != s.ip_hdr || s.ip_hdr < 20u || s.tcp_hdr < 20u || s.tcp_hdr > 60u ||
        (s.tcp_hdr & 3u) || s.ip_hdr + s.tcp_hdr > T)
        return false;
    s.v6 = ip.v6;
    s.seq = m[1];
    s.ack = m[2];
    s.window = m[4] & 0xffffu;
    s.flags = misc & 0xffu;
    s.key[0] = s.v6 ? s.h[2] : s.h[3];
    s.key[1] = s.v6 ? s.h[3] : 0u;
    s.key[2] = s.v6 ? s.h[4] : 0u;
    s.key[3] = s.v6 ? s.h[5] : 0u;
    s.key[4] = m[3];  // sport | dport << 16
    s.key[5] = s.v6 ? 6u : 4u;
    return true;
}

// The listen table's entry for the segment's destination port, RNS_UDP_NO_SOCK if nobody listens there.
__device__ __forceinline__ uint32_t listen_sock(const ListenArgs &a, const ListenSeg &s)
{
    const uint32_t l = a.n_listen ? a.listen[s.key[4] >> 16] : RNS_UDP_NO_SOCK;
    return l < a.n_listen ? l : RNS_UDP_NO_SOCK;
}

// Whether resident r's key is k.  (r comes out of the table, which this call alone writes; it is checked like
// any other input all the same.)
__device__ __forceinline__ bool listen_same(const ListenArgs &a, uint32_t r, const uint32_t (&k)[6])
{
    if (r >= a.rx.n)
        return false;
    ListenSeg o;
    if (!listen_seg(a, r, listen_gi(a.rx, r), o))
        return false;
    return o.key[0] == k[0] && o.key[1] == k[1] && o.key[2] == k[2] && o.key[3] == k[3] && o.key[4] == k[4] &&
           o.key[5] == k[5];
}

constexpr uint32_t kListenEmpty = 0xffffffffu;        // a slot's first after the clear
constexpr unsigned long long kListenEmpty64 = ~0ull;  // a slot's (resident, tag) after the clear: no resident is 2^32 - 1

// Whether the slot word r (resident | tag << 32) stands for key k of hash h, asked by datagram p.
__device__ __forceinline__ bool listen_match(const ListenArgs &a, unsigned long long r, uint32_t h, uint32_t p, const uint32_t (&k)[6])
{
    const uint32_t res = static_cast<uint32_t>(r);
    return static_cast<uint32_t>(r >> 32) == h && (res == p || listen_same(a, res, k));
}

__global__ __launch_bounds__(kScanBlock) void listen_classify_kernel(const ListenArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t blk = blockIdx.x * kListenWaves + (threadIdx.x >> 6);
    const PoolLane e = pool_lane(a.rx, blk, lane);
    if (!e.live)
        return;
    ListenSeg s;
    uint32_t rec = 0;
    if (listen_seg(a, e.p, e.gi, s)) {
        const bool cand = (s.flags & 0x02u) && listen_sock(a, s) != RNS_UDP_NO_SOCK;
        rec = RNS_CONN_UNMATCHED | (s.v6 ? 0u : kListenRecV4) | (cand ? kListenRecCand : 0u);
        if (cand) {
            const uint32_t p = static_cast<uint32_t>(e.p);
            const uint64_t smask = a.slots - 1u;
            const uint32_t h = flow_hash(s.key);
            const unsigned long long mine = p | (static_cast<unsigned long long>(h) << 32);
            uint64_t at = h & smask;
            for (uint64_t t = 0; t < a.slots; ++t) {
                const unsigned long long r = atomicCAS(a.tbl + at, kListenEmpty64, mine);
                if (r == kListenEmpty64 || listen_match(a, r, h, p, s.key)) {
                    atomicMin(a.first + at, p);
                    break;
                }
                at = (at + 1u) & smask;
            }
        }
    }
    a.w.rec[e.p] = rec;
}

// s(key): the smallest candidate index of key k in the batch, kListenEmpty if it has none.  p: the asking
// datagram, which is its own key's resident more often than not.
__device__ __forceinline__ uint32_t listen_first(const ListenArgs &a, uint32_t p, const uint32_t (&k)[6])
{
    const uint64_t smask = a.slots - 1u;
    const uint32_t h = flow_hash(k);
    uint64_t at = h & smask;
    for (uint64_t t = 0; t < a.slots; ++t) {
        const unsigned long long r = a.tbl[at];
        if (r == kListenEmpty64)
            break;
        if (listen_match(a, r, h, p, k))
            return a.first[at];
        at = (at + 1u) & smask;
    }
    return kListenEmpty;
}

// parse_options (tcp.rs:856-892) over the header bytes [20, tcp_hdr) of the first buffer: false where the
// reference does not return — an option's length byte past the end (it panics), a length of 0 (it loops for
// ever), a type 2 with fewer than 4 bytes left (it panics).  At most 40 bytes, so at most 40 steps.
__device__ __forceinline__ bool listen_options(const ListenSeg &s, uint32_t &mss)
{
    const uint8_t *o = reinterpret_cast<const uint8_t *>(s.h) + s.ip_hdr + 20u;
    const uint32_t n = s.tcp_hdr - 20u;
    mss = 0;
    uint32_t at = 0;
    while (at < n) {
        const uint32_t type = o[at];
        if (type == 0u)
            break;
        if (type == 1u) {
            at += 1u;
            continue;
        }
        if (at + 1u >= n)
            return false;
        const uint32_t len = o[at + 1u];
        if (type == 2u) {
            if (at + 4u > n)
                return false;
            mss = (static_cast<uint32_t>(o[at + 2u]) << 8) | o[at + 3u];
        }
        if (len == 0u)
            return false;
        at += len;
    }
    return true;
}

__global__ __launch_bounds__(kScanBlock) void listen_resolve_kernel(const ListenArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t blk = blockIdx.x * kListenWaves + (threadIdx.x >> 6);
    const PoolLane e = pool_lane(a.rx, blk, lane);
    uint32_t rec = e.live ? a.w.rec[e.p] : 0u;
    ListenSeg s;
    if ((rec & RNS_CONN_UNMATCHED) && listen_seg(a, e.p, e.gi, s)) {  // (the classify found it so: the same inputs)
        const uint32_t p = static_cast<uint32_t>(e.p);
        const uint32_t first = listen_first(a, p, s.key);
        if (first < p) {
            rec |= RNS_CONN_LATER;
        } else if (rec & kListenRecCand) {  // first == p: the key's first SYN
            uint32_t mss;
            rec |= listen_options(s, mss) ? RNS_CONN_SYN | (mss << kListenRecMssShift) : RNS_CONN_HOST;
        } else {
            rec |= RNS_CONN_RST;
        }
    } else {
        rec = 0;
    }
    if (e.live)
        a.w.rec[e.p] = rec;
    const uint32_t reply = (rec & (RNS_CONN_SYN | RNS_CONN_RST)) ? 1u : 0u;
    uint2 ta, tb;
    (void)scan2_block(make_uint2(reply, (reply && (rec & kListenRecV4)) ? 1u : 0u), ta);
    (void)scan2_block(make_uint2((rec & RNS_CONN_SYN) ? 1u : 0u, 0u), tb);
    if (threadIdx.x == 0) {
        a.w.part_a[blockIdx.x] = ta;
        a.w.part_b[blockIdx.x] = tb;
    }
}

// A reply's head, composed and stored by one lane: send_packet / the RST of tcp.rs:582-595 -> tcp_output ->
// ip_output_v4 / ip_output_v6.  IPD = the IP header's dwords.  Every dword but the two that hold a checksum is
// stored as it is summed.
template <uint32_t IPD>
__device__ __forceinline__ void listen_head(const LocalAddrs &local, const ListenSeg &s, uint32_t *o, bool syn, uint32_t seq,
                                            uint32_t id)
{
    constexpr bool v4 = IPD == 5u;
    const uint32_t tcplen = syn ? 24u : 20u;
    uint32_t d[IPD + 5u];
    if constexpr (v4) {
        d[0] = 0x45u | (bswap16_u32(20u + tcplen) << 16);
        d[1] = bswap16_u32(id);
        d[2] = 0x0640u;
        d[3] = local.v4;
        d[4] = s.key[0];
    } else {
        d[0] = 0x60u;
        d[1] = bswap16_u32(tcplen) | (6u << 16) | (64u << 24);
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            d[2u + k] = local.v6[k];
            d[6u + k] = s.key[k];
        }
    }
    const uint32_t ports = s.key[4];  // the segment's sport | dport << 16: the reply's source port is its dport
    d[IPD] = bswap16_u32(ports >> 16) | (bswap16_u32(ports & 0xffffu) << 16);
    d[IPD + 1u] = __builtin_bswap32(seq);
    d[IPD + 2u] = __builtin_bswap32(s.seq + 1u);
    d[IPD + 3u] = syn ? 0x60u | (0x12u << 8) | (0xffffu << 16) : 0x50u | (0x14u << 8);
    d[IPD + 4u] = 0u;
    const uint32_t opt = 0xdc050402u;  // 02 04 05 dc: MSS 1500
    TcpHeadSum hs;
#pragma unroll
    for (uint32_t k = 0; k < IPD + 5u; ++k) {
        hs.add(k, d[k], v4, IPD);
        if (k != IPD + 4u && !(v4 && k == 2u))
            o[k] = d[k];
    }
    if (syn) {
        hs.tcp += be2(opt);
        o[IPD + 5u] = opt;
    }
    if constexpr (v4)
        o[2] = d[2] | (bswap16_u32(hs.ip_csum()) << 16);
    o[IPD + 4u] = bswap16_u32(hs.l4_head(tcplen) ^ 0xffffu);  // tcp.rs:957-973, no payload
}

__global__ __launch_bounds__(kScanBlock) void listen_build_kernel(const ListenArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t blk = blockIdx.x * kListenWaves + (threadIdx.x >> 6);
    const PoolLane e = pool_lane(a.rx, blk, lane);
    const uint32_t rec = e.live ? a.w.rec[e.p] : 0u;
    const bool syn = (rec & RNS_CONN_SYN) != 0, reply = (rec & (RNS_CONN_SYN | RNS_CONN_RST)) != 0;
    const bool v4 = (rec & kListenRecV4) != 0;
    uint2 ta, tb;
    const uint2 xa = scan2_block(make_uint2(reply ? 1u : 0u, (reply && v4) ? 1u : 0u), ta);
    const uint2 xb = scan2_block(make_uint2(syn ? 1u : 0u, 0u), tb);
    const uint2 ca = a.w.part_a[blockIdx.x], cb = a.w.part_b[blockIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the totals, whatever reply_cap is
        const uint2 na = a.w.part_a[gridDim.x], nb = a.w.part_b[gridDim.x];
        a.count[0] = na.x;
        a.count[1] = na.y;
        a.count[2] = nb.x;
    }
    if (!e.live)
        return;
    const uint32_t k = ca.x + xa.x, v4_before = ca.y + xa.y, acc = cb.x + xb.x;  // acc <= k
    const bool built = reply && k < a.reply_cap;
    a.conn[e.p] = static_cast<uint8_t>((rec & 0x7fu) | (!reply ? 0u : built ? RNS_CONN_BUILT : RNS_CONN_NOBUF));
    ListenSeg s;
    if (!built || !listen_seg(a, e.p, e.gi, s))  // (a reply: the classify found it so)
        return;
    const uint32_t hl = (v4 ? 40u : 60u) + (syn ? 4u : 0u);
    a.rep_src[k] = static_cast<uint32_t>(e.p);
    a.rep_len8[k] = static_cast<uint8_t>(hl);
    const uint32_t seq = syn ? a.iss[acc] : 1u;
    uint32_t *o = reinterpret_cast<uint32_t *>(a.out + 64ull * k);
    if (v4)
        listen_head<5u>(a.local, s, o, syn, seq, ip_id(a.ip_id_base, a.ip_id_add, v4_before));
    else
        listen_head<10u>(a.local, s, o, syn, seq, 0u);
    if (!syn)
        return;
    // handle_new_connection: the key it inserts, the socket it leaves
    uint32_t *r = a.accept + 18ull * acc;
#pragma unroll
    for (uint32_t j = 0; j < 6u; ++j)
        r[j] = s.key[j];
    r[6] = s.seq + 1u;   // rcv_nxt
    r[7] = s.seq + 1u;   // rcv_max
    r[8] = s.seq;        // snd_una: send_unacked = seq_num (tcp.rs:917), the peer's number, as the reference has it
    r[9] = seq;          // snd_nxt
    r[10] = s.window;    // snd_wnd
    r[11] = s.seq;       // snd_wl1
    r[12] = s.ack;       // snd_wl2
    r[13] = 0u;
    r[14] = 0u;
    r[15] = RNS_TCP_SYN_RECEIVED << 16;
    r[16] = static_cast<uint32_t>(e.p);
    r[17] = listen_sock(a, s) | ((rec >> kListenRecMssShift) << 16);
}

}  // namespace rns
